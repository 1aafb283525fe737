"""GPU: every route of the dense bottleneck between encoder and decoder (AE / VAE / ceVAE), on the fp64 oracle.  The host side picks, per handle shape
(csrc/uad_bott.hip, csrc/uad_model.hip):

* U or fused (uad_bottleneck_fused_ok): a chain of generic 1x1 / dense launches + reparam kernels, or one kernel per direction.  Refusals: zDim not a
  multiple of 16, more than 1024 head columns (2 zDim for the VAEs), 1024 not a multiple of the head columns or of zDim (the non-power-of-two latents),
  the slice rule (zDim has to split over the k-groups in steps of 16), the 150 KiB LDS cap;
* Q1 or Q4 (uad_bottleneck_group): one workgroup per sample, or four that exchange partial vectors through global memory; the 1024 threads of a workgroup
  form 1024 / (slice width) k-groups over a feature slice narrower than 1024;
* w or g (uad_bottleneck_wgrad_ok): every parameter gradient in one fused launch (64 samples per chunk), or four filter-gradient GEMMs + column sums.

BOTT_CASES holds the smallest supported shapes that reach each route and each sub-case.  Each runs one whole step through tests/step_parity.py's flip-aware
body (reconstruction, loss scalars, the latent outputs z_mu / z_log_sigma / z_sigma or z, and EVERY gradient tensor against oracle/vae.py differentiated with the device's
activation pattern) at the project's own bars -- gpu_util.REL_TOL = 1e-4, its flip bound and flip cap -- in 'f32', and one case per route in 'bf16x3' too
(the bottleneck arithmetic is fp32 in every mode; the mode changes what feeds it).  The route a case runs is READ from the library
(Engine.debug_plan('bott', 0, 'B', n): computed by the launchers' own decision functions, nothing launched) and has to be the one the table names: a
changed rule moves a case off its route and fails here before it can hide.  test_bottleneck_census shows that the table reaches every decision."""
import pytest

pytestmark = pytest.mark.gpu

try:
    from tests.step_parity import check_capacity, make_engine, step
except Exception:
    make_engine = None

# (arch, height, inter_res, zdim, n, route) -- route: U | Q<workgroups per sample><w fused parameter gradients | g GEMMs>, as the library reports it
BOTT_CASES = [
    ('VAE', 32, 8, 48, 5, 'U'),           # non-power-of-two latent
    ('AE', 32, 8, 96, 3, 'U'),
    ('ceVAE', 32, 8, 48, 3, 'U'),
    ('VAE', 32, 8, 16, 65, 'U'),          # slice rule; ragged past 64 rows: conv2d's bias column sum runs in 17 row chunks, the generic filter gradients split
    ('VAE', 32, 8, 1024, 2, 'U'),         # 2048 head columns
    ('AE', 128, 32, 512, 2, 'U'),         # 152 KiB of LDS in the backward
    ('AE', 32, 8, 32, 65, 'Q1g'),         # 2 k-groups
    ('VAE', 32, 4, 64, 3, 'Q1w'),         # 4 k-groups
    ('AE', 64, 4, 128, 2, 'Q1w'),
    ('VAE', 64, 16, 32, 3, 'Q4g'),        # 2 k-groups
    ('AE', 128, 16, 16, 2, 'Q4g'),        # slice of 1024: 1 k-group
    ('ceVAE', 64, 16, 32, 2, 'Q4g'),
    ('VAE', 32, 8, 128, 65, 'Q4w'),       # 8 k-groups; 65 rows: two chunks of the fused parameter-gradient kernel, one row in the last
    ('VAE', 32, 4, 256, 3, 'Q4w'),        # 16 k-groups
    ('VAE', 64, 16, 64, 2, 'Q4w'),        # 2 k-groups
    ('VAE', 128, 16, 128, 2, 'Q4w'),      # slice of 1024
    ('VAE', 128, 32, 256, 3, 'Q4w'),      # slice of 2048; the backward's LDS exactly at the 150 KiB cap
    ('VAE', 64, 8, 512, 3, 'Q4w'),        # 1024 head columns: one k-group in the heads; 4 k-groups over the slice
    ('AE', 64, 8, 1024, 2, 'Q4w'),
]
# one case per route in 'bf16x3' as well
BF16X3_CASES = {('VAE', 32, 8, 48, 5), ('AE', 32, 8, 32, 65), ('VAE', 32, 4, 64, 3), ('VAE', 64, 16, 32, 3), ('VAE', 64, 8, 512, 3)}
RUNS = [(c, m) for c in BOTT_CASES for m in (('f32', 'bf16x3') if c[:5] in BF16X3_CASES else ('f32',))]


def route(p):
    return 'U' if not p['fused'] else f'Q{p["wgs"]}{"w" if p["fused_wgrad"] == 1 else "g"}'


def _id(c):
    return '-'.join(str(v) for v in c)


@pytest.mark.parametrize('case,math', RUNS, ids=[f'{_id(c)}-{m}' for c, m in RUNS])
def test_bottleneck_route_meets_the_oracle(case, math):
    arch, h, inter, zdim, n, want = case
    s = step(arch, h, n, zdim=zdim, inter=inter)
    eng = make_engine(arch, h, n, zdim=zdim, inter=inter)
    try:
        eng.set_params(s.p32)
        eng.set_math(math)
        p = eng.debug_plan('bott', 0, 'B', n)
        assert route(p) == want, f'{s.tag}: the library runs this shape on {route(p)}, the table says {want}: {p}'
        s.run(eng, math, leg=f'bottleneck {want}')
    finally:
        eng.close()


# ---------------------------------------------------------------- census
# Decisions no supported (height, inter_res, zDim) reaches, each with its reason (none so far).
UNREACHABLE = {}


def _heads(c):
    return c[3] * (1 if c[0] == 'AE' else 2)


def _pow2(v):
    return v & (v - 1) == 0


# predicates over (report, case).  The report does not name the reason of a refusal, so the refusal entries classify by the case: every size but zDim is a
# power of two in a supported handle, so an unfused power-of-two latent with at most 1024 head columns was refused either by the slice rule (zDim does not
# split over the reported k-groups in steps of 16) or, failing that, by the LDS cap.
WANTED = {
    'U': lambda p, c: route(p) == 'U',
    'Q1g': lambda p, c: route(p) == 'Q1g',
    'Q1w': lambda p, c: route(p) == 'Q1w',
    'Q4g': lambda p, c: route(p) == 'Q4g',
    'Q4w': lambda p, c: route(p) == 'Q4w',
    'Q4, 1 k-group': lambda p, c: p['fused'] and p['wgs'] == 4 and p['kgroups'] == 1,
    'Q4, 2 k-groups': lambda p, c: p['fused'] and p['wgs'] == 4 and p['kgroups'] == 2,
    'Q4, 4 k-groups': lambda p, c: p['fused'] and p['wgs'] == 4 and p['kgroups'] == 4,
    'Q4, 8 k-groups': lambda p, c: p['fused'] and p['wgs'] == 4 and p['kgroups'] == 8,
    'Q4, 16 k-groups': lambda p, c: p['fused'] and p['wgs'] == 4 and p['kgroups'] == 16,
    'Q1, 2 k-groups': lambda p, c: p['fused'] and p['wgs'] == 1 and p['kgroups'] == 2,
    'Q1, 4 k-groups': lambda p, c: p['fused'] and p['wgs'] == 1 and p['kgroups'] == 4,
    'backward LDS exactly at the cap': lambda p, c: p['fused'] and p['lds_bwd'] == 150 * 1024,
    'refused by the LDS cap': lambda p, c: not p['fused'] and _pow2(c[3]) and _heads(c) <= 1024 and c[3] % (16 * p['kgroups']) == 0,
    'refused by the slice rule': lambda p, c: not p['fused'] and _pow2(c[3]) and _heads(c) <= 1024 and c[3] % (16 * p['kgroups']) != 0,
    'refused by more than 1024 head columns': lambda p, c: not p['fused'] and _pow2(c[3]) and _heads(c) > 1024,
    'refused by a non-power-of-two zDim': lambda p, c: not p['fused'] and not _pow2(c[3]),
    'fused parameter gradients, more than one chunk, short last chunk': lambda p, c: p['fused_wgrad'] == 1 and p['wgrad_chunks'] > 1 and p['wgrad_last_rows'] < 64,
    'a bias column sum in more than one row chunk (GEMM parameter gradients)': lambda p, c: p['fused_wgrad'] != 1 and p['cs_need'] > 0,
}


def test_bottleneck_census():
    """Host only (one handle per case is created and closed; nothing is launched): the report of every BOTT_CASES handle at its batch.  Every entry of WANTED
    has to be hit by at least one case or be named in UNREACHABLE; every case has to sit on the route the table names; the plain arithmetic of the report is
    checked against the case; and at every n up to the case's batch the bottleneck's slabs and column-sum scratch fit what uad_create allocated
    (step_parity.check_capacity; that the row can fail is test_bottleneck_capacity_check_can_fail's business).  Run with -s for the census."""
    seen = {w: [] for w in WANTED}
    for c in BOTT_CASES:
        arch, h, inter, zdim, n, want = c
        eng = make_engine(arch, h, n, zdim=zdim, inter=inter)
        try:
            p = eng.debug_plan('bott', 0, 'B', n)
            print(f'{_id(c[:5]):22s} {route(p):3s} {p}')
            assert route(p) == want, f'{_id(c)}: the library reports {route(p)}: {p}'
            rows = n * (2 if arch == 'ceVAE' else 1)
            assert (p['wgrad_chunks'], p['wgrad_last_rows']) == ((rows + 63) // 64, rows - 64 * ((rows + 63) // 64 - 1)), p
            assert (p['lds_fwd'] == 0 and p['lds_bwd'] == 0) if not p['fused'] else (0 < p['lds_fwd'] <= 150 * 1024 and 0 < p['lds_bwd'] <= 150 * 1024), p
            assert p['wgs'] in (1, 4) and p['fused_wgrad'] == (-1 if not p['fused'] else p['fused_wgrad']) and p['fused_wgrad'] in (-1, 0, 1), p
            for k in range(1, n + 1):
                check_capacity(eng, k)
            for w, hit in WANTED.items():
                if hit(p, c):
                    seen[w].append(_id(c[:5]))
        finally:
            eng.close()
    missing = []
    for w, where in seen.items():
        print(f'{w}: {len(where)} cases' + (f', first {where[0]}' if where else (' -- UNREACHABLE: ' + UNREACHABLE[w] if w in UNREACHABLE else ' -- MISSING')))
        if not where and w not in UNREACHABLE:
            missing.append(w)
        assert not (where and w in UNREACHABLE), f'{w} is listed as unreachable but occurs at {where[0]}'
    assert not missing, f'no case reaches: {missing}'


def test_bottleneck_capacity_check_can_fail():
    """check_capacity's bottleneck row can fail (the row on its own: kinds = 'B').  The slab allocation is shared with the 5x5 layers, whose need dwarfs the
    bottleneck's at this shape, so half of it still holds; against a capacity far below one filter the row has to object."""
    arch, h, inter, zdim, n, _ = BOTT_CASES[3]
    eng = make_engine(arch, h, n, zdim=zdim, inter=inter)
    try:
        cap = eng.debug_plan('bott', 0, 'B', n)['cap']
        with pytest.raises(AssertionError, match='filter-gradient slab floats|column-sum scratch floats') as e:
            for shrink in (2, 1 << 20):
                for k in range(1, n + 1):
                    check_capacity(eng, k, shrink=shrink, kinds='B')
        print(f'\n[shrunk capacity {cap}] {e.value}')
    finally:
        eng.close()


def test_bottleneck_plan_refused_without_a_bottleneck():
    eng = make_engine('GMVAE_spatial', 256, 1)
    try:
        with pytest.raises(ValueError, match='no dense bottleneck'):
            eng.debug_plan('bott', 0, 'B', 1)
    finally:
        eng.close()
