"""CPU: the host statement of NII.normalize(method='standardization') (utils/standardize.py; reference utils/NII.py:53-75).  The ordered fp64
sums are held to the exactly rounded sums of the same float32 terms (math.fsum) within the chain bound include/uad_hip.h states; the
statement and numpy's own float32 evaluation are both held to the expression in fp64 within the bound DESIGN §25 derives from one float32
rounding of each scalar."""
import math
import os
import re

import numpy as np
import pytest

from tests import standardize_cases as sc
from unsupervised_anomaly_detection_brain_mri_amd.utils import standardize as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def held_to_fsum(v, **kw):
    u, q = st.shifted_terms(v, **kw)
    got = st.shifted_sums(v, **kw)
    for g, terms in zip(got, (u, q)):
        t64 = terms.astype(np.float64)
        exact, bar = math.fsum(t64), st.SUM_CHAIN * sc.U64 * math.fsum(np.abs(t64))
        print(f'n = {terms.size} {kw}: sum {g!r}, exact {exact!r}, |diff| {abs(g - exact):.3e}, bound {bar:.3e}')
        assert abs(g - exact) <= bar, (terms.size, kw, g, exact, bar)


@pytest.mark.parametrize('n', sc.SIZES)
def test_ordered_sums_against_the_exactly_rounded_sums(n):
    v = sc.values(n)
    held_to_fsum(v)
    mean32 = np.float32(st.shifted_sums(v)[0] / n)
    held_to_fsum(v, shift=mean32)
    held_to_fsum(v, clamp_lo=-100.0, clamp_hi=650.0, shift=mean32, centre=np.float32(3e-6))
    held_to_fsum(sc.offset_values(n), shift=np.float32(1e4), centre=np.float32(-1e-4))


def test_the_order_is_the_stated_one():
    """Against a scalar loop over the stated order (thread runs, tree, strided runs, tree) at a size with a ragged last tile."""
    n = 2 * sc.T + 77
    x = sc.values(n).astype(np.float64)

    def tree(r):
        r, d = list(r), 128
        while d >= 1:
            for t in range(d):
                r[t] = r[t] + r[t + d]
            d //= 2
        return r[0]
    partials = []
    for tile in range(-(-n // sc.T)):
        runs = []
        for t in range(256):
            s = 0.0
            for r in range(8):
                for e in range(4):
                    j = tile * sc.T + (r * 256 + t) * 4 + e
                    if j < n:
                        s = s + float(x[j])
            runs.append(s)
        partials.append(tree(runs))
    runs = []
    for t in range(256):
        s = 0.0
        for p in range(t, len(partials), 256):
            s = s + partials[p]
        runs.append(s)
    assert float(st.ordered_sum(x)) == tree(runs)


def test_the_chain_is_what_the_header_states():
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'uad_hip.h')).read()
    chain = int(re.search(r'UAD_SHIFTED_SUMS_CHAIN\s*=\s*(\d+)', header).group(1))
    assert chain == _lib.SHIFTED_SUMS_CHAIN == st.SUM_CHAIN == st.sum_chain(st.MAX_N) == 32 + 8 + 1024 + 8
    assert all(st.sum_chain(n) <= chain for n in sc.SIZES)


def test_two_passes_hold_where_one_pass_fails():
    """1e4 + 1e-2 * noise: E[x^2] - E[x]^2 from float32 squares has lost the variance; the centred form has not."""
    v = sc.offset_values(13 * 17 * 19)
    n = v.size
    x = v.astype(np.float64)
    exact = math.sqrt(math.fsum((x - math.fsum(x) / n) ** 2) / n)
    _, (mean32, std32) = st.standardize(v, None, None, return_moments=True)
    s1, s2 = st.shifted_sums(v)
    one_pass = s2 / n - (s1 / n) ** 2
    print(f'exact std {exact!r}, statement {float(std32)!r}, one-pass variance {one_pass!r} (exact variance {exact * exact!r})')
    assert abs(float(std32) - exact) <= 4 * sc.U32 * exact
    assert abs(float(mean32) - math.fsum(x) / n) <= sc.U32 * 1e4 * 1.001
    assert not abs(one_pass - exact * exact) <= 0.5 * exact * exact


@pytest.mark.parametrize('lower,upper', [(None, None), (0, 99.8), (5, 95)])
@pytest.mark.parametrize('kind', ['volume', 'offset'])
def test_statement_and_numpy_within_the_derived_bound_of_fp64(kind, lower, upper):
    v = sc.values(13 * 17 * 19).reshape(13, 17, 19) if kind == 'volume' else sc.offset_values(13 * 17 * 19)
    clamped, ref = sc.numpy_float32(v, lower, upper)
    got = st.standardize(v, lower, upper)
    assert got.dtype == np.float32 and got.shape == v.shape
    O, bar = sc.bound(clamped)
    e_ref, e_got = np.abs(ref.reshape(-1) - O), np.abs(got.reshape(-1) - O)
    print(f'{kind} {lower} {upper}: numpy / bound {np.max(e_ref / bar):.3f}, statement / bound {np.max(e_got / bar):.3f}, largest bound {bar.max():.3e}')
    assert np.all(e_ref <= bar), 'the reference itself leaves the bound'
    assert np.all(e_got <= bar)


def test_clamped_form_equals_the_percentile_form():
    v = sc.values(13 * 17 * 19)
    lo, hi = np.percentile(v, 5), None
    w = v.copy(); w[w < lo] = lo
    hi = np.percentile(w, 95)
    assert st.standardize_clamped(v, lo, hi).tobytes() == st.standardize(v, 5, 95).tobytes()


def test_constant_volume_is_all_nan_as_in_numpy():
    v = np.full((3, 5, 7), 0.75, np.float32)                     # float32 adds 105 x 0.75 exactly: numpy's mean is the value, c == 0
    _, ref = sc.numpy_float32(v)
    got, (mean32, std32) = st.standardize(v, 0, 99.8, return_moments=True)
    assert mean32 == 0.75 and std32 == 0.0 and np.isnan(ref).all() and np.isnan(got).all()
    # where numpy's float32 mean of a constant is not the constant, its c is a non-zero constant and c / 0 is an infinity: never finite
    v = np.full((3, 5, 7), 0.7310586, np.float32)
    _, ref = sc.numpy_float32(v)
    got, (mean32, std32) = st.standardize(v, 0, 99.8, return_moments=True)
    assert mean32 == v.flat[0] and std32 == 0.0 and np.isnan(got).all() and not np.isfinite(ref).any()


def test_empty_input_and_the_sign_of_a_zero_sum():
    assert st.shifted_sums(np.zeros(0, np.float32)) == (0.0, 0.0)
    assert float(st.ordered_sum(np.array([-0.0]))) == 0.0 and not np.signbit(st.ordered_sum(np.array([-0.0])))
