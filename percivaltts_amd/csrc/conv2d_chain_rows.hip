// The per-row form of the Conv2D chain kernels (ptts_conv2d_chain_*_rows: zero-padded batches with a length per row) in a
// translation unit of its own: the ROWS = true instantiations of conv2d_chain.hip's kernel templates and the entry points that
// launch them.  Why not one unit: see the top of that file.
#define PTTS_CHAIN_ROWS 1
#include "conv2d_chain.hip"
