"""Curvature-flow denoising of a volume: the host statement of `nii.denoise()` (utils/NII.py:85-87,
`sitk.CurvatureFlow(image1, timeStep=0.125, numberOfIterations=3)`), which the reference's MS datasets call on every volume right after
reading it (dataloaders/MSLUB.py:242, MSISBI2015.py:231, MSSEG2008.py:241,246).

The arithmetic is ITK's CurvatureFlowFunction::ComputeUpdate and DenseFiniteDifferenceImageFilter::ApplyUpdate written down from their
source; nobody has compared it with SimpleITK's output yet (SimpleITK is not a dependency of this project).

One iteration is a Jacobi sweep over the fp64 volume u[z, y, x].  ITK numbers the dimensions x = 0, y = 1, z = 2 and, with image spacing
in use and a neighbourhood of radius 1, scales the differences of dimension i by a_i = 1 / spacing_i.  Neighbours beyond the volume follow
the zero-flux Neumann rule: every index is clamped to its own axis (edge replication, corners included).  With p(d) the clamped neighbour
at offset d and c = p(0):

    f[i]    = (0.5 * (p(+e_i) - p(-e_i))) * a_i
    s[i]    = ((p(+e_i) - 2 c) + p(-e_i)) * (a_i * a_i)
    x[i][j] = ((0.25 * (((p(-e_i-e_j) - p(-e_i+e_j)) - p(+e_i-e_j)) + p(+e_i+e_j))) * a_i) * a_j          (i < j)
    mag     = ((0 + f0 f0) + f1 f1) + f2 f2
    upd     = 0 where mag < 1e-9, otherwise
              (sum_i (sum_{j != i} s[j]) * (f[i] f[i])  -  sum_{i<j} ((2 f[i]) * f[j]) * x[i][j]) / mag
    u'      = c + upd * time_step

Every operation is one IEEE fp64 add, multiply or divide in the order written (sums run left to right from 0.0), with no fused
multiply-add -- numpy has none -- so that the device kernel (csrc/uad_flow.hip, device_ops.DeviceOps.curvature_flow), which is compiled with
contraction off, returns the same bits.  This module is the reference every test of that kernel compares against, and the path
nifti.volume_to_slices takes when no device engine is given."""
import numpy as np


def curvature_flow(vol, spacing=(1, 1, 1), time_step=0.125, iterations=3):
    """-> float64 [z, y, x]; spacing = (sx, sy, sz), positive and finite.  iterations = 0 returns a copy.  The input is not modified."""
    u = np.array(vol, np.float64)
    if u.ndim != 3 or 0 in u.shape:
        raise ValueError(f'vol must be a non-empty [z, y, x] volume, got shape {u.shape}')
    sp = np.asarray(spacing, np.float64)
    if sp.shape != (3,) or not np.all(np.isfinite(sp)) or not np.all(sp > 0):
        raise ValueError(f'spacing must be three positive finite numbers (x, y, z), got {spacing!r}')
    if int(iterations) != iterations or iterations < 0:
        raise ValueError(f'iterations must be a non-negative integer, got {iterations!r}')
    a = [np.float64(1.0) / s for s in sp]                       # a[i], i = 0 (x), 1 (y), 2 (z)
    ts = np.float64(time_step)
    for _ in range(int(iterations)):
        u = _sweep(u, a, ts)
    return u


_SLAB_VOXELS = 1 << 22          # the sweep keeps about twenty temporaries: z slabs of this many voxels bound them at a few hundred MB


def _sweep(u, a, ts):
    p = np.pad(u, 1, mode='edge')
    out = np.empty_like(u)
    slab = max(1, _SLAB_VOXELS // (u.shape[1] * u.shape[2]))
    for z0 in range(0, u.shape[0], slab):
        z1 = min(z0 + slab, u.shape[0])
        out[z0:z1] = _sweep_padded(p[z0:z1 + 2], a, ts)          # elementwise in the output voxel: slabs change no bit
    return out


def _sweep_padded(p, a, ts):
    """One sweep over the interior of an edge-padded block p [nz + 2, ny + 2, nx + 2] -> [nz, ny, nx]."""
    n = tuple(k - 2 for k in p.shape)

    def tap(dx=0, dy=0, dz=0):
        return p[1 + dz:1 + dz + n[0], 1 + dy:1 + dy + n[1], 1 + dx:1 + dx + n[2]]

    def off(i, si, j=None, sj=0):
        d = [0, 0, 0]
        d[i] = si
        if j is not None:
            d[j] = sj
        return tap(*d)

    c = tap()
    f, s, x = [None] * 3, [None] * 3, {}
    mag = np.zeros(n)
    for i in range(3):
        f[i] = (0.5 * (off(i, 1) - off(i, -1))) * a[i]
        s[i] = ((off(i, 1) - 2.0 * c) + off(i, -1)) * (a[i] * a[i])
        for j in range(i + 1, 3):
            x[i, j] = ((0.25 * (((off(i, -1, j, -1) - off(i, -1, j, 1)) - off(i, 1, j, -1)) + off(i, 1, j, 1))) * a[i]) * a[j]
        mag = mag + f[i] * f[i]
    upd = np.zeros(n)
    for i in range(3):
        t = np.zeros(n)
        for j in range(3):
            if j != i:
                t = t + s[j]
        upd = upd + t * (f[i] * f[i])
    for i in range(3):
        for j in range(i + 1, 3):
            upd = upd - ((2.0 * f[i]) * f[j]) * x[i, j]
    gate = mag < 1e-9
    with np.errstate(divide='ignore', invalid='ignore'):
        upd = np.where(gate, 0.0, upd / mag)
    return c + upd * ts
