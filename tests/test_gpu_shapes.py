"""GPU: planner coverage, on the fp64 oracle.  The host-side planner picks different kernels / split factors as the batch and the image size change
(spatial vs generic implicit GEMM, channel-chunk splits reduced in the kernel or by a second launch, the 64- / 32-column instance, the fused final
epilogue, the bf16x6 three-plane route or its exact-fp32 fall-back, the filter gradient's tile splits with an even or a short last split).  For a sweep
of ragged batch sizes and resolutions, in all three math modes on one handle, with the three dropout sites live:

* reconstruction, loss scalars and EVERY gradient tensor are held to the fp64 oracle (oracle/vae.py) at the project's bar -- 1e-4 max-norm relative in
  'f32' and 'bf16x3', 1e-5 in 'bf16x6' -- flip-aware: the activation pattern the device used is read back (tests/gpu_util.py:
  device_activation_pattern), every disagreement with the oracle has to be a rounding tie of the mode (FLIP_BOUND) and their number stays under the scale
  tests' cap, and the oracle is differentiated with the device's pattern (tests/step_parity.py holds the body; tests/test_gpu_handle_reuse.py runs the
  same body on one handle stepped through a batch sequence);
* the two independent kernel families still have to agree with EACH OTHER as this file always asked: reconstruction and loss of 'bf16x3' against 'f32'
  at 1e-4, gradients at relative L2 3e-2 and max-norm 1e-1, the ceVAE anomaly map at L2 3e-2.  Those mode-vs-mode gradient bounds are gross-error nets
  only (a few flipped activations move single entries of the small dense gradients by 1e-3 between ANY two fp32 implementations); the bar on the
  gradients is the oracle comparison above;
* test_plan_census shows (uad_debug_plan, nothing launched) that the cases of the two files reach every value of the planner's decisions, or names the
  value in UNREACHABLE with the reason."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:
    from tests.gpu_util import assert_close
    from tests.step_parity import MODES, REUSE_CASES, SHAPE_CASES, make_engine, planned_blocks, step
except Exception:
    make_engine = None


@pytest.mark.parametrize('arch,h,n', SHAPE_CASES)
def test_math_modes_agree_across_planner_paths(arch, h, n):
    s = step(arch, h, n)
    eng = make_engine(arch, h, n)
    eng.set_params(s.p32)
    res = {}
    for math in MODES:
        eng.set_math(math)
        r = s.run(eng, math)
        res[math] = (r.bits['x_hat'].cpu().numpy(), r.bits['scalars'].cpu().numpy(), eng.get_grads(),
                     r.bits['anomaly'].cpu().numpy() if arch == 'ceVAE' else None)
    eng.close()
    # mode against mode, as before the oracle comparison existed
    xa, sa, ga, aa = res['f32']
    xb, sb, gb, ab = res['bf16x3']
    assert_close(xb, xa, name='x_hat')
    assert abs(sb[2] - sa[2]) <= 1e-4 * abs(sa[2])
    for name, _, _ in s.m.spec:
        a64, b64 = ga[name].astype(np.float64), gb[name].astype(np.float64)
        l2 = np.linalg.norm(b64 - a64) / max(np.linalg.norm(a64), 1e-30)
        assert l2 <= 3e-2, f'{name}: relative L2 {l2:.2e}'
        assert_close(gb[name], ga[name], tol=1e-1, name=name)
    if aa is not None:
        l2 = np.linalg.norm(ab.astype(np.float64) - aa) / np.linalg.norm(aa.astype(np.float64))
        assert l2 <= 3e-2, f'anomaly: relative L2 {l2:.2e}'


# ---------------------------------------------------------------- plan census
# Values of the planner's decisions no supported shape of the sweep can reach, each with its reason (reviewed, not silently empty).
UNREACHABLE = {
    'generic filter gradient': 'every planned block (encoder 1.., decoder 0..) has 32 | CB, 32 | CS and, at the handles\' inter_res = 8, HS = WS >= 8 a multiple of 8, so choose_w5 '
                               'always takes it; the generic kernel computes the bottleneck\'s dense / 1x1 filter gradients (no planned block) and is held per contraction by '
                               'tests/test_gpu_ops.py / test_gpu_ops_large.py through uad_op_conv_w',
}

WANTED = {
    'FD': {'spatial unsplit': lambda p: p['path'] == 1 and p['splits'] == 1,
           'spatial split, slabs reduced in the kernel': lambda p: p['path'] == 1 and p['splits'] > 1 and p['inkernel'] == 1,
           'spatial split, separate epilogue launch': lambda p: p['path'] == 1 and p['splits'] > 1 and p['inkernel'] == 0,
           'split-K generic': lambda p: p['path'] == 2,
           'plain generic': lambda p: p['path'] == 0,
           '64-column instance': lambda p: p['path'] == 1 and p['colblock'] == 64,
           '32-column instance': lambda p: p['path'] == 1 and p['colblock'] == 32,
           'bf16x6 three-plane route taken': lambda p: p['x6'] == 1,
           'bf16x6 route refused (exact-fp32 fall-back)': lambda p: p['x6'] == 0,
           'fused final taken': lambda p: p['fused_final'] == 1,
           'fused final refused': lambda p: p['fused_final'] == 0},
    'W': {'choose_w5, even last split': lambda p: p['kernel'] == 1 and p['splits'] > 1 and p['short_last'] == 0,
          'choose_w5, short last split': lambda p: p['kernel'] == 1 and p['short_last'] == 1,
          'choose_w5, one 32-channel block per workgroup': lambda p: p['kernel'] == 1 and p['csblocks'] == 1,
          'choose_w5, two 32-channel blocks per workgroup': lambda p: p['kernel'] == 1 and p['csblocks'] == 2,
          'generic filter gradient': lambda p: p['kernel'] == 0},
}


def test_plan_census():
    """Host only (the library has to be loaded and a handle created; nothing is launched): walks every (handle, batch) the two files run, in the three math
    modes, and collects the distinct plans per kind.  Every value in WANTED has to occur, or be named in UNREACHABLE.  Run with -s for the census."""
    walks = [(a, h, n, (n,)) for a, h, n in SHAPE_CASES] + [(a, h, mb, tuple(sorted(set(seq)))) for a, h, mb, seq in REUSE_CASES]
    seen = {(k, w): [] for k in WANTED for w in WANTED[k]}
    plans = {}
    for arch, h, mb, ns in walks:
        eng = make_engine(arch, h, mb)
        for math in MODES:
            eng.set_math(math)
            for n in ns:
                for side, layer, kind in planned_blocks(eng):
                    p = eng.debug_plan(side, layer, kind, n)
                    fam = 'W' if kind == 'W' else 'FD'
                    sig = tuple(v for k, v in p.items() if k not in ('need', 'cap', 'cp_need', 'cp_cap', 'tiles', 'units', 'units_per_split'))
                    plans.setdefault((kind, math), {}).setdefault(sig, f'{arch} {h} max_batch {mb} n={n} {side}{layer}')
                    for w, hit in WANTED[fam].items():
                        if hit(p):
                            seen[(fam, w)].append(f'{arch} {h} n={n} (max_batch {mb}) {math} {side}{layer}.{kind}')
        eng.close()
    for (kind, math), d in sorted(plans.items()):
        print(f'\n[{kind} {math}] {len(d)} distinct plans')
        for sig, first in sorted(d.items()):
            print(f'    {sig}  first at {first}')
    missing = []
    for (fam, w), where in seen.items():
        print(f'{fam:2s} {w}: {len(where)} launches' + (f', first {where[0]}' if where else (' -- UNREACHABLE: ' + UNREACHABLE[w] if w in UNREACHABLE else ' -- MISSING')))
        if not where and w not in UNREACHABLE:
            missing.append(w)
        assert not (where and w in UNREACHABLE), f'{w} is listed as unreachable but occurs at {where[0]}'
    assert not missing, f'the sweep reaches no plan with: {missing}'
