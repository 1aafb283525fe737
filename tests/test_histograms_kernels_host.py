"""CPU: the kernels of csrc/uad_hist.hip (uad_histogram_by_class: hist_class_kernel, hist_class_finish_kernel) against the host statement,
without a GPU -- tests/native/hist_emu.cpp compiles the kernel source itself for the host with -ffp-contract=off, runs every workgroup's
threads as real threads around a std::barrier and drives them with the library's launch geometry.  Counts must EQUAL np.histogram of every
class on the shared table; the fp64 sums are held to the exactly rounded values (math.fsum) at the bar of the GPU test, must not change
by a bit with the grid, and every tile's partial must have been written (the workspace is poisoned).  Shapes and inputs are those of
tests/test_gpu_histograms.py (tests/hist_cases.py).  The masked select shares the select kernel, whose wave intrinsics have no host form:
it is covered on the device."""
import os
import subprocess

import numpy as np
import pytest

from tests import hist_cases as hc
from tests.emu_build import build_emu
from unsupervised_anomaly_detection_brain_mri_amd.utils.order_stats import edges_to_float32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'hist_emu', 'uad_hist.hip')
    d = os.path.dirname(exe)
    f = lambda name: os.path.join(d, name)

    def run(v, lab, n_classes, edges32=None, centre=None, moments=True, in_off=0, lab_off=0, max_blocks=0):
        np.ascontiguousarray(v, np.float32).tofile(f('in.f32'))
        np.ascontiguousarray(lab, np.uint8).tofile(f('lab.u8'))
        bins = 0 if edges32 is None else len(edges32) - 1
        if bins:
            np.ascontiguousarray(edges32, np.float32).tofile(f('edges.f32'))
        if centre is not None:
            np.ascontiguousarray(centre, np.float64).tofile(f('centre.f64'))
        subprocess.run([exe, f('in.f32'), f('lab.u8'), str(len(v)), str(n_classes), f('edges.f32') if bins else '-', str(bins),
                        f('centre.f64') if centre is not None else '-', str(int(moments)), str(in_off), str(lab_off), str(max_blocks), f('out.bin')], check=True)
        raw = np.fromfile(f('out.bin'), np.int64)
        counts = raw[:n_classes * bins].reshape(n_classes, bins)
        if not moments:
            return counts, None, None
        return counts, raw[n_classes * bins:n_classes * bins + n_classes], raw[n_classes * bins + n_classes:].view(np.float64)
    return run


def two_pass(emu, v, lab, k, edges32, **kw):
    _, cnt, sums = emu(v, lab, k, **kw)
    with np.errstate(invalid='ignore'):                                   # a class without a value (n below the number of classes): 0 / 0
        mean = sums / cnt
        counts, cnt2, sq = emu(v, lab, k, edges32=edges32, centre=mean, **kw)
        assert np.array_equal(cnt, cnt2)
        return counts, cnt, mean, sq / cnt


@pytest.mark.parametrize('n', hc.SIZES)
def test_counts_and_moments_per_class(emu, n):
    for k in hc.CLASSES:
        lab = hc.ids(n, k, extra=True)
        for kind, bins in zip(hc.KINDS, (50, 1024, 2, 1, 50, 50)):
            v = hc.values(kind, n, lab, bins)
            e32 = edges_to_float32(hc.edge_table(bins))
            counts, cnt, mean, var = two_pass(emu, v, lab, k, e32, in_off=n % 4, lab_off=(n + k) % 3)
            assert np.array_equal(counts, hc.reference_counts(v, lab, k, e32)), (k, kind, bins)
            for c, exact in enumerate(hc.exact_moments(v, lab, k)):
                d = v[lab == c].astype(np.float64)
                if exact is not None:
                    assert hc.moments_hold(cnt[c], mean[c], var[c], exact), (k, kind, c, mean[c], var[c], exact)
                elif d.size:                                              # an infinity in the class: numpy's inf / nan
                    with np.errstate(invalid='ignore'):
                        assert cnt[c] == d.size and np.array_equal(mean[c], np.mean(d), equal_nan=True) and np.isnan(var[c]), (k, kind, c)


def test_float64_edges_fold_onto_float32_ones_that_bin_alike(emu):
    n, k = 3 * hc.T + 17, 2
    lab = hc.ids(n, k)
    v = hc.values('edges', n, lab, 50)
    e64 = hc.edge_table(50, dtype=np.float64)
    v[:51] = e64.astype(np.float32)                                       # float32 neighbours of the float64 edges
    counts, _, _ = emu(v, lab, k, edges32=edges_to_float32(e64), moments=False)
    assert np.array_equal(counts, hc.reference_counts(v.astype(np.float64), lab, k, e64))


def test_sums_do_not_depend_on_the_grid_or_the_alignment(emu):
    n, k = 3 * hc.T + 17, 4
    lab = hc.ids(n, k)
    v = hc.values('random', n, lab)
    base = emu(v, lab, k)
    for kw in (dict(max_blocks=1), dict(max_blocks=3), dict(lab_off=1), dict(lab_off=2)):
        got = emu(v, lab, k, **kw)
        assert got[1].tobytes() == base[1].tobytes() and got[2].tobytes() == base[2].tobytes(), kw
    # a shifted start moves every value to another thread's run: the sums may differ in the last bits, the bar holds
    got = emu(v, lab, k, in_off=3)
    assert np.array_equal(got[1], base[1]) and np.allclose(got[2], base[2], rtol=1e-13, atol=0)


def test_the_chain_of_dependent_additions_is_what_the_header_states():
    from unsupervised_anomaly_detection_brain_mri_amd import _lib
    import re
    header = open(os.path.join(ROOT, 'include', 'uad_hip.h')).read()
    chain = int(re.search(r'UAD_HISTOGRAM_SUM_CHAIN\s*=\s*(\d+)', header).group(1))
    tiles = ((2 ** 31 - 1) + 3 + hc.T - 1) // hc.T
    assert chain == _lib.HISTOGRAM_SUM_CHAIN == 32 + 8 + -(-tiles // 256) + 8 and chain <= hc.CHAIN_MAX
    assert chain * 2.0 ** -53 < hc.MOMENT_BAR
