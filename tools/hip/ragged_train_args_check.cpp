// Host-side check of the masked-training entry points: workspace queries and argument refusals, which return before any launch
// and never touch a device.  Built stand-alone with the host code under AddressSanitizer / UBSan:
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -I include \
//       tools/hip/ragged_train_args_check.cpp percivaltts_amd/csrc/{core,elementwise,evalcosts,lstm,gru}.hip -o ragged_train_args_check
// Exit status 0 and "ok" when every call answered as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "percival_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s (last error: %s)\n", __LINE__, #cond, ptts_last_error()); ++failures; } \
    } while (0)

int main() {
    float* p = reinterpret_cast<float*>(256);        // non-null, never dereferenced on the host
    double* d = reinterpret_cast<double*>(256);
    int* l = reinterpret_cast<int*>(256);
    const size_t big = (size_t)1 << 40;
    const int EINVAL_ = -1, EWORKSPACE_ = -3;

    // workspace queries: the dense sibling's size for the same [rows, C], 0 for what the calls refuse
    EXPECT(ptts_colstats_rows_workspace_bytes(4, 12, 256, 256) == ptts_colstats_workspace_bytes(48, 256));
    EXPECT(ptts_colstats_rows_workspace_bytes(3, 9, 20, 4) == ptts_colstats_workspace_bytes(135, 4));
    EXPECT(ptts_colstats_rows_workspace_bytes(64, 400, 65 * 4, 4) == ptts_colstats_workspace_bytes(64LL * 400 * 65, 4));
    EXPECT(ptts_colstats_rows_workspace_bytes(0, 12, 4, 4) == 0 && ptts_colstats_rows_workspace_bytes(4, 12, 6, 4) == 0);
    EXPECT(ptts_colstats_rows_workspace_bytes(4, -1, 4, 4) == 0 && ptts_colstats_rows_workspace_bytes(4, 12, 4, 0) == 0);

    // colstats_rows
    EXPECT(ptts_colstats_rows(nullptr, l, 4, 12, 4, 4, d, p, big, nullptr) == EINVAL_);
    EXPECT(ptts_colstats_rows(p, nullptr, 4, 12, 4, 4, d, p, big, nullptr) == EINVAL_);
    EXPECT(ptts_colstats_rows(p, l, 4, 12, 4, 4, nullptr, p, big, nullptr) == EINVAL_);
    EXPECT(ptts_colstats_rows(p, l, 0, 12, 4, 4, d, p, big, nullptr) == EINVAL_);
    EXPECT(ptts_colstats_rows(p, l, 4, 12, 6, 4, d, p, big, nullptr) == EINVAL_ && std::strstr(ptts_last_error(), "multiple"));
    for (int C : {3, 4, 256, 4096}) {
        const size_t need = ptts_colstats_rows_workspace_bytes(4, 12, C, C);
        EXPECT(need > 0);
        EXPECT(ptts_colstats_rows(p, l, 4, 12, C, C, d, p, 15, nullptr) == EWORKSPACE_);      // (the query covers either reduction path: only a size below both is refused for certain)
        EXPECT(ptts_colstats_rows(p, l, 4, 12, C, C, d, nullptr, need, nullptr) == EWORKSPACE_);
        EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, p, p, d, l, p, 15, 4, 12, C, C, 1, 0.3f, nullptr) == EWORKSPACE_);
    }
    // affine_act_rows_bwd_params
    EXPECT(ptts_affine_act_rows_bwd_params(nullptr, p, p, p, p, d, l, p, big, 4, 12, 4, 4, 1, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, nullptr, p, p, p, d, l, p, big, 4, 12, 4, 4, 0, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, p, nullptr, d, l, p, big, 4, 12, 4, 4, 1, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, p, p, nullptr, l, p, big, 4, 12, 4, 4, 1, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, nullptr, p, d, l, p, big, 4, 12, 4, 4, 1, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, p, p, d, l, p, big, 4, 12, 4, 4, 2, 0.3f, nullptr) == EINVAL_);
    EXPECT(ptts_affine_act_rows_bwd_params(p, p, p, p, p, d, l, p, big, 4, 12, 5, 4, 1, 0.3f, nullptr) == EINVAL_);
    // axpby_cols_rows
    EXPECT(ptts_axpby_cols_rows(nullptr, p, p, p, p, l, 4, 12, 4, 4, nullptr) == EINVAL_);
    EXPECT(ptts_axpby_cols_rows(p, p, nullptr, p, p, l, 4, 12, 4, 4, nullptr) == EINVAL_);
    EXPECT(ptts_axpby_cols_rows(p, p, p, p, p, nullptr, 4, 12, 4, 4, nullptr) == EINVAL_);
    EXPECT(ptts_axpby_cols_rows(p, p, p, p, p, l, 4, 0, 4, 4, nullptr) == EINVAL_);
    EXPECT(ptts_axpby_cols_rows(p, p, p, p, p, l, 4, 12, 7, 4, nullptr) == EINVAL_);
    // the costs: N has to lie in 1 .. B*T
    EXPECT(ptts_rows_combine(p, l, 4, 12, 0, p, nullptr) == EINVAL_ && ptts_rows_combine(p, l, 4, 12, 49, p, nullptr) == EINVAL_);
    EXPECT(ptts_rows_combine(nullptr, l, 4, 12, 10, p, nullptr) == EINVAL_ && ptts_rows_combine(p, l, 4, 12, 10, nullptr, nullptr) == EINVAL_);
    EXPECT(ptts_rows_mean_bwd(p, l, 4, 12, 1, 1.f, 0, p, nullptr) == EINVAL_ && ptts_rows_mean_bwd(p, l, 4, 12, 1, 1.f, 49, p, nullptr) == EINVAL_);
    EXPECT(ptts_rows_mean_bwd(p, nullptr, 4, 12, 1, 1.f, 10, p, nullptr) == EINVAL_ && ptts_rows_mean_bwd(p, l, 4, 12, 0, 1.f, 10, p, nullptr) == EINVAL_);
    EXPECT(ptts_wlse_rows_bwd(p, p, p, p, l, 4, 12, 7, 49, p, nullptr) == EINVAL_ && ptts_wlse_rows_bwd(p, nullptr, p, p, l, 4, 12, 7, 10, p, nullptr) == EINVAL_);
    EXPECT(ptts_wlse_rows_bwd(p, p, p, p, l, 4, 12, 7, 10, nullptr, nullptr) == EINVAL_ && ptts_wlse_rows_bwd(p, p, p, p, l, 0, 12, 7, 10, p, nullptr) == EINVAL_);
    // the recurrences' ragged backward: the dense backward's refusals, and lens
    for (int H : {5, 48, 64, 192, 256}) {
        for (int nd : {1, 2}) {
            const size_t nl = ptts_lstm_bwd_workspace_bytes(4, 12, H, nd), ng = ptts_gru_bwd_workspace_bytes(4, 12, H, nd);
            EXPECT(ptts_lstm_bwd_ragged(p, p, p, p, p, l, p, nl - 1, 4, 12, H, nd, 0, nullptr) == EWORKSPACE_);
            EXPECT(ptts_lstm_bwd_ragged(p, p, p, p, p, l, nullptr, nl, 4, 12, H, nd, 0, nullptr) == EWORKSPACE_);
            EXPECT(ptts_lstm_bwd_ragged(p, p, p, p, p, nullptr, p, nl, 4, 12, H, nd, 0, nullptr) == EINVAL_);
            EXPECT(ptts_gru_bwd_ragged(p, p, p, p, p, l, p, ng - 1, 4, 12, H, nd, nullptr) == EWORKSPACE_);
            EXPECT(ptts_gru_bwd_ragged(p, p, p, p, p, nullptr, p, ng, 4, 12, H, nd, nullptr) == EINVAL_);
        }
    }
    EXPECT(ptts_lstm_bwd_ragged(p, p, nullptr, p, p, l, p, big, 4, 12, 8, 1, 0, nullptr) == EINVAL_);
    EXPECT(ptts_lstm_bwd_ragged(p, p, p, p, p, l, p, big, 4, 12, 8, 3, 0, nullptr) == EINVAL_);
    EXPECT(ptts_lstm_bwd_ragged(p, p, p, p, p, l, p, big, 4, 12, 1025, 1, 0, nullptr) == EINVAL_);
    EXPECT(ptts_gru_bwd_ragged(p, p, p, nullptr, p, l, p, big, 4, 12, 8, 1, nullptr) == EINVAL_);
    EXPECT(ptts_gru_bwd_ragged(p, p, p, p, p, l, p, big, 4, 0, 8, 1, nullptr) == EINVAL_);
    std::printf(failures ? "%d check(s) failed\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
