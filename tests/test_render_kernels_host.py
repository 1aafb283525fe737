"""CPU: the arithmetic, the workgroup reduction, the resident / two-sweep paths and the store paths of the kernels of csrc/uad_render.hip
(uad_render_minmax_u8, uad_render_heatmap, uad_render_overlay) against the host statement utils/render.py, without a GPU --
tests/native/render_emu.cpp compiles the kernel source itself for the host with -ffp-contract=off, runs every workgroup's threads as real
threads around a std::barrier and drives them with the library's launch geometry.  Grey and overlay must be BIT-EQUAL; the heat map
INDEX-EQUAL without exemption: both sides call the C library's exp (utils/render.py goes through math.exp for that reason).  The emulator
puts the output between guard bytes and fails when one is written, and poisons the LDS structs before every workgroup.  Shapes and inputs
are those of tests/test_gpu_render.py (tests/render_cases.py)."""
import os
import subprocess

import numpy as np
import pytest

from tests import render_cases as rc
from tests.emu_build import build_emu
from unsupervised_anomaly_detection_brain_mri_amd.utils import render


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'render_emu', 'uad_render.hip')
    d = os.path.dirname(exe)
    f = lambda name: os.path.join(d, name)

    def grey(x, in_off=0, out_off=0):
        n, h, w = x.shape
        np.ascontiguousarray(x, np.float32).tofile(f('x.f32'))
        subprocess.run([exe, 'grey', f('x.f32'), *map(str, (n, h * w, in_off, out_off)), f('out.u8')], check=True)
        return np.fromfile(f('out.u8'), np.uint8).reshape(n, h, w)

    def heat(d_, lut, in_off=0, out_off=0):
        n, h, w = d_.shape
        np.ascontiguousarray(d_, np.float32).tofile(f('d.f32'))
        np.ascontiguousarray(lut, np.uint8).tofile(f('lut.u8'))
        subprocess.run([exe, 'heat', f('d.f32'), *map(str, (n, h, w)), f('lut.u8'), str(in_off), str(out_off), f('out.u8')], check=True)
        return np.fromfile(f('out.u8'), np.uint8).reshape(n, h, w, 4)

    def overlay(x, pred, gt, in_off=0, out_off=0):
        n, h, w = x.shape
        np.ascontiguousarray(x, np.float32).tofile(f('x.f32'))
        np.ascontiguousarray(pred, np.float32).tofile(f('p.f32'))
        np.ascontiguousarray(gt, np.uint8).tofile(f('g.u8'))
        subprocess.run([exe, 'overlay', f('x.f32'), f('p.f32'), f('g.u8'), *map(str, (n, h * w, in_off, out_off)), f('out.u8')], check=True)
        return np.fromfile(f('out.u8'), np.uint8).reshape(n, h, w, 3)
    return grey, heat, overlay


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_grey_kernel_has_the_bytes_of_the_host_statement(emu, case):
    n, hw = case
    for kind in rc.GREY_KINDS if n < rc.N_FOLD else ('uniform',):
        assert np.array_equal(emu[0](rc.grey_input(n, hw, kind)), rc.grey_reference(n, hw, kind)), kind
    if n == 1:
        # a base that is only 4-byte aligned takes single loads, an output off its dword takes byte stores
        assert np.array_equal(emu[0](rc.grey_input(n, hw, 'uniform'), in_off=1), rc.grey_reference(n, hw, 'uniform'))
        assert np.array_equal(emu[0](rc.grey_input(n, hw, 'uniform'), out_off=1), rc.grey_reference(n, hw, 'uniform'))


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_heat_map_kernel_has_the_indices_of_the_host_statement(emu, case):
    n, hw = case
    for kind in rc.HEAT_KINDS if n < rc.N_FOLD else ('lesions',):
        got = emu[1](rc.heat_input(n, hw, kind), rc.INDEX_LUT)
        assert np.array_equal(got[..., 0], rc.heat_reference_index(n, hw, kind)), kind
        assert np.array_equal(got, rc.INDEX_LUT[got[..., 0]]), kind                                  # the four bytes of the entry, in order
    if n == 1:
        ref = render.heatmap_rgba(rc.heat_input(n, hw, 'lesions'))                                   # the jet table
        assert np.array_equal(emu[1](rc.heat_input(n, hw, 'lesions'), render.jet_u8()), ref)
        assert np.array_equal(emu[1](rc.heat_input(n, hw, 'lesions'), render.jet_u8(), in_off=1), ref)
        assert np.array_equal(emu[1](rc.heat_input(n, hw, 'lesions'), render.jet_u8(), out_off=4), ref)       # dword stores instead of 16 bytes


@pytest.mark.parametrize('case', rc.CASES, ids=rc.case_id)
def test_overlay_kernel_has_the_bytes_of_the_host_statement(emu, case):
    n, hw = case
    x, pred, gt = rc.overlay_input(n, hw)
    assert np.array_equal(emu[2](x, pred, gt), rc.overlay_reference(n, hw))
    if n == 1:
        assert np.array_equal(emu[2](x, pred, gt, in_off=1), rc.overlay_reference(n, hw))
        assert np.array_equal(emu[2](x, pred, gt, out_off=1), rc.overlay_reference(n, hw))


def test_the_exemption_cap_holds_when_exp_moves_by_an_ulp(monkeypatch):
    """The GPU test lets a heat-map pixel differ by one index where the statement's q * 256 lies within 1e-9 of an integer and caps such
    pixels at 0.1 %.  Checked here before relying on it: the statement with every exp() nudged one ulp up, and one ulp down, stays inside
    the exemption on the GPU test's inputs and moves far fewer pixels than the cap."""
    real = render._exp
    total = moved = 0
    for direction in (np.inf, -np.inf):
        monkeypatch.setattr(render, '_exp', lambda t, d=direction: np.nextafter(real(t), d))
        for n, hw in rc.CASES:
            if n >= rc.N_FOLD:
                continue
            nudged = render.heatmap_index(rc.heat_input(n, hw, 'lesions'))
            differ, uncovered = rc.heat_mismatch(nudged, rc.heat_q256(n, hw, 'lesions'))
            assert uncovered == 0, (n, hw, direction, differ)
            moved += differ
            total += nudged.size
    monkeypatch.setattr(render, '_exp', real)
    print(f'exp nudged by one ulp: {moved} of {total} heat-map pixels change their index')
    assert moved <= rc.EXEMPT_CAP * total
