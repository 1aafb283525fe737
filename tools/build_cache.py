"""Builds a slice cache (utils/slice_cache.py) from a directory of NIfTI volumes laid out like the reference's MS datasets
(dataloaders/MSLUB.py:277-322): <root>/<patient>/<patient>_<PROTOCOL>.nii.gz, <patient>_consensus_gt.nii.gz, <patient>_brainmask.nii.gz.

    python tools/build_cache.py <root> <cache_dir> --protocol FLAIR --res 128 --start 15 --end 125

The volume -> slice steps are those of utils/nifti.py (skull stripping, percentile scaling, empty-slice filter, pad / zoom).
--curvature-flow [ITER STEP] applies the curvature-flow denoising of the reference loaders (nii.denoise(), utils/NII.py:85-87; without
values: 3 iterations of time step 0.125) to every volume before skull stripping, with the voxel spacing of its header; on the device
(uad_curvature_flow) when an engine is used, else utils/curvature_flow.py on the host -- the same bits.  That arithmetic is ITK's update
written down from its source and has not been compared with SimpleITK's own output.  --device-resample runs the pad / zoom step's cubic spline on the GPU;
--device-stats also runs the percentile scaling and the empty-slice filter there (one upload per volume, resampled slices come back).
--rotations A [A ...]: the rotation augmentation of the reference's dataset classes (dataloaders/BRAINWEB.py:156-162), one cached slice per
angle; with a device engine the rotations run there too (uad_affine_spline3).  The default, 0, caches the unrotated slices only.
--loader brainweb prepares the volumes the way the reference prepares its BrainWeb training set (dataloaders/BRAINWEB.py:125-185, 266-292;
nifti.volume_to_slices(loader='brainweb')) instead of the MS datasets' way: --gt then names the TISSUE-CLASS file (values 0 .. 10), which
supplies the skull map and the lesion map (== 10), and --mask is ignored; constant slices are dropped; a slice larger than --res is resized
as cv2.resize does (bilinear image, nearest label; utils/resize.py, not compared with OpenCV itself, which is not a dependency), a smaller
one zero-padded.  --no-skull-removal keeps FAT / MUSCLE / SKIN / SKULL / CONNECTIVE, --no-background-removal keeps BACKGROUND.  With a device
engine (--device-resample or --device-stats) the whole path runs on the GPU (uad_mask_by_label, uad_select_quantiles, uad_resize2d).
--curvature-flow is refused for this loader: the reference does not denoise BrainWeb.
--crops {center,lesions,random} W H caches crops instead of whole slices, the reference's `useCrops` with its cropType, cropWidth and cropHeight
(dataloaders/MSLUB.py:186-222, BRAINWEB.py:165-180; nifti.volume_to_slices(crops=...), utils/crops.py): the centre crop, one crop per lesion
of the label slice centred on its centroid (not with --rotations), or --random-crops-per-slice N windows per slice whose corners come from a
numpy RandomState seeded with --crop-seed S (one stream over all patients; the label map is cropped at the image's origins).  With a device
engine the component measurements and the window gather run on the GPU (uad_cc_label, uad_cc_props, uad_crop2d) -- the same crops bit for bit.
--normalization {scaling,standardization}: NII.normalize's method (utils/NII.py:53-75).  'scaling', the default, is what the reference's
configurations use; 'standardization' is the default its loaders declare (MSLUB.py:49, BRAINWEB.py:55): the same percentile clamp, then
(v - mean) / std over the whole volume (utils/standardize.py; with a device engine uad_shifted_sums and uad_clamp_standardize, same bits).
The cached values are then not in [0, 1].
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unsupervised_anomaly_detection_brain_mri_amd.utils import nifti  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('root'); ap.add_argument('cache')
    ap.add_argument('--protocol', default='FLAIR')
    ap.add_argument('--gt', default='consensus_gt'); ap.add_argument('--mask', default='brainmask')
    ap.add_argument('--res', type=int, default=128); ap.add_argument('--axis', default='axial')
    ap.add_argument('--start', type=int, default=0); ap.add_argument('--end', type=int, default=155)
    ap.add_argument('--train', type=float, default=0.7); ap.add_argument('--val', type=float, default=0.2); ap.add_argument('--test', type=float, default=0.1)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device-resample', action='store_true', help='resample the slices with the device spline op (uad_zoom_spline3) instead of scipy')
    ap.add_argument('--device-stats', action='store_true',
                    help='percentile scaling and empty-slice filter on the device select op (uad_select_quantiles); implies --device-resample')
    ap.add_argument('--rotations', type=float, nargs='+', default=[0], metavar='A',
                    help='angles in degrees, one cached slice per angle and kept slice (0 = unrotated; on the device when an engine is used)')
    ap.add_argument('--curvature-flow', nargs='*', default=None, metavar=('ITER', 'STEP'),
                    help='curvature-flow denoising before skull stripping; no values = 3 iterations of time step 0.125 (nii.denoise())')
    ap.add_argument('--loader', choices=('mslub', 'brainweb'), default='mslub',
                    help="'brainweb': the training set's preparation; --gt names the tissue-class file, --mask is ignored")
    ap.add_argument('--no-skull-removal', action='store_true', help='--loader brainweb: keep the skull tissue classes (4, 5, 6, 7, 9)')
    ap.add_argument('--no-background-removal', action='store_true', help='--loader brainweb: keep the background class (0)')
    ap.add_argument('--crops', nargs=3, default=None, metavar=('MODE', 'W', 'H'), help="cache crops of W x H (width, height): MODE center | lesions | random")
    ap.add_argument('--random-crops-per-slice', type=int, default=5, metavar='N', help='--crops random: windows per slice and angle (numRandomCropsPerSlice)')
    ap.add_argument('--crop-seed', type=int, default=0, metavar='S', help='--crops random: seed of the numpy RandomState the corners are drawn from')
    ap.add_argument('--normalization', choices=nifti.NORMALIZATIONS, default='scaling',
                    help="NII.normalize's method: 'scaling' (clamp, divide by the maximum) or 'standardization' (clamp, subtract the mean, divide by the std)")
    a = ap.parse_args()
    if a.curvature_flow is not None and len(a.curvature_flow) not in (0, 2):
        ap.error('--curvature-flow takes no values or ITER STEP')
    flow = None if a.curvature_flow is None else (True if not a.curvature_flow else (int(a.curvature_flow[0]), float(a.curvature_flow[1])))
    crops = {}
    if a.crops is not None:
        if a.crops[0] not in ('center', 'lesions', 'random'):
            ap.error('--crops MODE must be center, lesions or random')
        try:
            w, h = int(a.crops[1]), int(a.crops[2])
        except ValueError:
            ap.error('--crops W H must be integers')
        if a.crops[0] == 'lesions' and any(r != 0 for r in a.rotations):
            ap.error('--crops lesions does not go with --rotations')
        crops = {'crops': (a.crops[0], w, h)}
        if a.crops[0] == 'random':
            import numpy as np
            crops = {'crops': ('random', w, h, a.random_crops_per_slice), 'rng': np.random.RandomState(a.crop_seed)}
    patients = []
    for name in sorted(os.listdir(a.root)):
        d = os.path.join(a.root, name)
        vol = os.path.join(d, f'{name}_{a.protocol}.nii.gz')
        if not os.path.isfile(vol):
            continue
        gt, mk = os.path.join(d, f'{name}_{a.gt}.nii.gz'), os.path.join(d, f'{name}_{a.mask}.nii.gz')
        if a.loader == 'brainweb':
            mk = ''                                                    # the tissue classes are the skull map
        patients.append({'name': name, 'volume': vol, 'groundtruth': gt if os.path.isfile(gt) else None, 'skullmap': mk if os.path.isfile(mk) else None})
    if not patients:
        raise SystemExit(f'no <patient>/<patient>_{a.protocol}.nii.gz under {a.root}')
    loader = {}
    if a.loader == 'brainweb':
        if flow is not None:
            ap.error('--curvature-flow does not go with --loader brainweb')
        loader = {'loader': 'brainweb', 'skull_removal': not a.no_skull_removal, 'background_removal': not a.no_background_removal}
    engine = None
    if a.device_resample or a.device_stats:
        from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
        engine = DeviceOps()       # the model-independent device ops: ingestion needs no model
    info = nifti.build_cache(a.cache, patients, partition={'TRAIN': a.train, 'VAL': a.val, 'TEST': a.test}, seed=a.seed, engine=engine, axis=a.axis,
                             slice_start=a.start, slice_end=a.end, slice_resolution=(a.res, a.res), **({'rotations': tuple(a.rotations)} if list(a.rotations) != [0] else {}),
                             **({'device_stats': a.device_stats} if engine is not None and not loader else {}), **({'curvature_flow': flow} if flow is not None else {}),
                             **loader, **crops, **({'normalization': a.normalization} if a.normalization != 'scaling' else {}))
    print(json.dumps(info))


if __name__ == '__main__':
    main()
