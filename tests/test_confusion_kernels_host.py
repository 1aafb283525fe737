"""CPU: the kernels of csrc/uad_confusion.hip (uad_confusion_by_segment: confusion_zero_kernel, confusion_kernel, confusion_tn_kernel) against
the host statement utils/confusion.py, without a GPU -- tests/native/confusion_emu.cpp compiles the kernel source itself for the host, runs
every workgroup's threads as real threads around a std::barrier and drives them with the library's launch geometry.  LDS is poisoned before
every workgroup and the counts hold garbage before the first launch.  The counts must EQUAL the statement's for every case of
tests/confusion_cases.py at both thresholds: with the library's grid (one workgroup per four tiles: one workgroup for the longest segment
of the cases, three tiles), with 1 and 2 workgroups per segment, where a workgroup strides over tiles and the atomics of two workgroups
meet, and with 3, one workgroup a tile."""
import os
import subprocess

import numpy as np
import pytest

from tests import confusion_cases as cc
from tests.emu_build import build_emu

GRIDS = (0, 1, 2, 3)                                         # workgroups per segment; 0 = the library's


@pytest.fixture(scope='module')
def emu(tmp_path_factory):
    exe = build_emu(tmp_path_factory, 'confusion_emu', 'uad_confusion.hip')
    d = os.path.dirname(exe)
    f = lambda name: os.path.join(d, name)

    def run(case, thr, grids=GRIDS):
        """-> int64 [len(grids), P, 4]"""
        case.pred.tofile(f('pred.f32'))
        case.gt.tofile(f('gt.u8'))
        case.offsets.tofile(f('offsets.i64'))
        subprocess.run([exe, f('pred.f32'), f('gt.u8'), str(case.pred.size), f('offsets.i64'), str(case.offsets.size - 1), repr(float(np.float32(thr))),
                        str(case.pred_shift), str(case.gt_shift), ','.join(str(g) for g in grids), f('out.bin')], check=True)
        return np.fromfile(f('out.bin'), np.int64).reshape(len(grids), -1, 4)
    return run


def emulated(cases):
    return [c for c in cases if c.pred.size]                  # n == 0 launches nothing: the entry point's business, not the kernels'


def check(emu, case):
    for thr in cc.THRESHOLDS:
        want = cc.statement(case, thr)
        got = emu(case, thr)
        assert got.dtype == want.dtype and got.shape == (len(GRIDS),) + want.shape
        for grid, g in zip(GRIDS, got):
            assert np.array_equal(g, want), (case.name, thr, grid, g.tolist(), want.tolist())
        assert np.array_equal(want.sum(axis=1), np.diff(case.offsets))


@pytest.mark.parametrize('case', emulated(cc.prefix_cases() + cc.small_cases() + cc.class_cases()), ids=lambda c: c.name)
def test_counts_equal_the_statement_on_every_grid(emu, case):
    check(emu, case)


def test_counts_equal_the_statement_for_every_base_alignment_on_every_grid(emu):
    cases = cc.shift_cases()
    assert {(c.pred_shift, c.gt_shift) for c in cases} == {(p, g) for p in range(4) for g in range(16)}
    want = cc.statement(cases[0], 0.5)                        # the same arrays behind every pair of shifts
    assert want[:, :3].min(initial=1, where=np.diff(cases[0].offsets)[:, None] > 8) > 0
    for case in cases:
        check(emu, case)
