"""What the fused Conv2D-stack kernels (csrc/conv2d_chain.hip) cost at the reference's spectrum width, F = 129 bins (three
frequency blocks per time tile), L = 8, T = 400.  One process; the sides of every comparison alternate inside each repetition;
HIP events after a warm-up of every shape; median with p10 .. p90 over the repetitions.

  (i)   per launch: the four chain passes at F = 129, B = 10 and B = 64
  (ii)  per critic step (critic_loss + backward, eager, one stream) with cfg.arch_critic_bf16 = 'chain' against True -- at this
        width True is the layer-wise bf16 form, the yardstick: the summed time of all ptts_conv2d* launches (_hip.KernelTimer)
        and the wall time (HIP events around the step, no timer active)
  (iii) the price of the recomputed block halos: the same passes at F = 65, B = 128 -- about the bins of F = 129, B = 64

python tools/chain_wide_probe.py [--reps N] [--only launches|steps] [--json FILE]      (--json: the figures as one JSON object)"""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from percivaltts_amd import ops, _hip, backend_hip

T, L = 400, 8


def pct(xs):
    xs = sorted(xs)
    q = lambda f: xs[min(len(xs) - 1, int(round(f * (len(xs) - 1))))]
    return {'median': round(q(0.5), 1), 'p10': round(q(0.1), 1), 'p90': round(q(0.9), 1), 'n': len(xs)}


def event_us(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(); fn(); e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3


def chain_passes(B, F, tab, g):
    """The four passes of one geometry as closures over their buffers."""
    FP = (F + 1) & ~1
    x0 = torch.randn(B, T, F, generator=g).cuda()
    maps = torch.empty((L - 1, B, T, FP, 4), dtype=torch.bfloat16, device='cuda')
    gmaps = torch.empty((L, B, T, FP, 4), dtype=torch.bfloat16, device='cuda')
    a_last = torch.empty((B, T, F, 4), dtype=torch.bfloat16, device='cuda')
    d16 = torch.randn(B, T, F, 4, generator=g).cuda().to(torch.bfloat16)
    g0 = torch.empty((B, T, F), device='cuda'); u0 = torch.randn(B, T, F, generator=g).cuda()
    o2 = torch.empty((B, T, F, 4), dtype=torch.bfloat16, device='cuda')
    parts = torch.empty(_hip.lib().ptts_conv2d_chain_partials_bytes(L), dtype=torch.uint8, device='cuda')
    nb, npart = ctypes.c_int(0), ctypes.c_int(0)
    P, st, call = _hip.ptr, _hip.stream, _hip.call
    keep = (x0, maps, gmaps, a_last, d16, g0, u0, o2, parts, nb, npart)
    return {
        'fwd': lambda: call('ptts_conv2d_chain_fwd', P(x0), x0.stride(1), P(tab), P(maps), P(a_last), B, T, F, L, 0.3, st()),
        'bwd': lambda: call('ptts_conv2d_chain_bwd', P(d16), 1, P(x0), x0.stride(1), P(maps), P(a_last), P(tab), P(parts), parts.numel(),
                            ctypes.byref(nb), ctypes.byref(npart), B, T, F, L, 1, 0.3, st()),
        'bwd_data+gamma': lambda: call('ptts_conv2d_chain_bwd_data', P(d16), 1, P(maps), P(a_last), P(tab), P(gmaps), P(g0), B, T, F, L, 0.3, st()),
        'second': lambda: call('ptts_conv2d_chain_second', P(u0), P(gmaps), P(maps), P(a_last), P(tab), P(o2), 1, P(parts), parts.numel(),
                               ctypes.byref(nb), ctypes.byref(npart), B, T, F, L, 1, 0.3, st()),
    }, keep


def launches(reps):
    g = torch.Generator().manual_seed(1)
    ws = [(torch.rand(5, 5, 1 if l == 0 else 4, 4, generator=g) - 0.5).mul(0.3).cuda() for l in range(L)]
    bs = [torch.zeros(4).cuda() for _ in range(L)]
    tab = ops._C2C.table(ws, bs)
    geos = [(10, 129), (64, 129), (128, 65)]
    sides = {geo: chain_passes(geo[0], geo[1], tab, g) for geo in geos}
    for geo in geos:                                 # warm-up of every shape (forward first: the other passes read its maps)
        for _ in range(3):
            for fn in sides[geo][0].values():
                fn()
    torch.cuda.synchronize()
    times = {geo: {k: [] for k in sides[geo][0]} for geo in geos}
    for _ in range(reps):
        for name in ('fwd', 'bwd', 'bwd_data+gamma', 'second'):
            for geo in geos:                         # the geometries alternate inside a repetition
                times[geo][name].append(event_us(sides[geo][0][name]))
    out = {}
    for geo in geos:
        nfb = _hip.lib().ptts_conv2d_chain_blocks(geo[1], L, None, None, None, 0)
        out['B{}_F{}'.format(*geo)] = dict({k: pct(v) for k, v in times[geo].items()}, blocks=nfb, bins=geo[0] * T * geo[1])
        print('B = {:3d}, F = {:3d} ({} block(s)), us per launch:'.format(geo[0], geo[1], nfb),
              {k: '{median} [{p10} .. {p90}]'.format(**pct(v)) for k, v in times[geo].items()}, flush=True)
    return out


def build(args, B, form, dev):
    """bench.build_optimizer's critic step at spec = 129 with cfg.arch_critic_bf16 = form (that function makes the option a bool)."""
    import io, contextlib
    from percivaltts_amd import vocoders, modeltts_common, networks_critic, optimizertts_wgan
    cfg = bench.make_cfg(args)
    cfg.train_batch_size = B
    cfg.arch_critic_bf16 = form
    cfg.train_wgan_bf16_products = True
    cfg.train_wgan_hipgraph = False
    cfg.train_wgan_parallel_streams = False
    cfg.train_wgan_prune_dead_branches = True; cfg.train_wgan_stack_real_fake = True; cfg.train_wgan_reuse_ctx_conv = True
    cfg.train_wgan_early_critic = True; cfg.train_wgan_split_bf16 = True
    voc = vocoders.VocoderPML(16000, 0.005, 129, 33)
    with contextlib.redirect_stdout(io.StringIO()):
        mod = modeltts_common.DCNNF0SpecNoiseFeatures(args.ctx, voc, cfg)
        crit = networks_critic.Critic(voc, args.ctx, cfg)
        opt = optimizertts_wgan.OptimizerTTSWGAN(cfg, mod, errtype=args.errtype, critic=crit)
        opt.prepare()
    X, Y = bench.synthetic(B, T, args.ctx, voc.featuressize(), 129, 123, dev)
    alpha = torch.rand(B, generator=torch.Generator().manual_seed(3)).to(dev)

    def step():
        opt.critic_opti.zero_grad()
        with ops.deferred_weight_grads():
            tot, _ = opt.critic_loss(X, Y, alpha, training=True)
            tot.backward()
    return step


def steps(reps):
    args = argparse.Namespace(batch=64, ctx=601, errtype='WLSWGAN')      # what bench.make_cfg / build() below read: bench.py's defaults
    dev = backend_hip.device()
    out = {}
    for B in (10, 64):
        forms = {'chain': build(args, B, 'chain', dev), 'layers (True)': build(args, B, True, dev)}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        wall = {k: [] for k in forms}; conv = {k: [] for k in forms}; ncalls = {}
        for _ in range(reps):
            for k, fn in forms.items():              # the two forms alternate inside a repetition
                wall[k].append(event_us(fn))
            for k, fn in forms.items():
                with _hip.KernelTimer() as kt:
                    fn()
                d = [r for r in kt.durations_ms() if r[0].startswith('ptts_conv2d')]
                conv[k].append(sum(r[2] for r in d) * 1e3); ncalls[k] = len(d)
        out['B{}'.format(B)] = {k: {'wall_us': pct(wall[k]), 'conv2d_launches_us': pct(conv[k]), 'conv2d_launches': ncalls[k]} for k in forms}
        for k in forms:
            print('critic step, B = {:3d}, F = 129, {:14s}: wall {median} [{p10} .. {p90}] us;'.format(B, k, **pct(wall[k])),
                  '{} ptts_conv2d* launches, {median} [{p10} .. {p90}] us'.format(ncalls[k], **pct(conv[k])), flush=True)
        c, l = out['B{}'.format(B)]['chain'], out['B{}'.format(B)]['layers (True)']
        for what in ('wall_us', 'conv2d_launches_us'):
            verdict = 'faster' if c[what]['p90'] < l[what]['p10'] else 'slower' if c[what]['p10'] > l[what]['p90'] else 'not separated'
            print('   {}: chain is {} (chain p90 {} vs layer-wise p10 {})'.format(what, verdict, c[what]['p90'], l[what]['p10']), flush=True)
        del forms
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--only', choices=['launches', 'steps'], default=None)
    ap.add_argument('--json', metavar='FILE', default=None)
    a = ap.parse_args()
    out = {}
    if a.only != 'steps':
        out['launches'] = launches(a.reps)
    if a.only != 'launches':
        out['critic_step'] = steps(a.reps)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
