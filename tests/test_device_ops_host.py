"""CPU: the model-independent device ops stand alone (device_ops.DeviceOps) and both engine families inherit them -- one implementation, no
second path -- and the public surface of the engines is the one recorded in tests/engine_surface.json BEFORE the ops and the handle plumbing
moved (`python tests/test_device_ops_host.py > tests/engine_surface.json` at that commit wrote it).  Importing the modules is enough: no
GPU and no library."""
import inspect
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from unsupervised_anomaly_detection_brain_mri_amd import engine, gan_engine  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.engine import Engine, Scores  # noqa: E402
from unsupervised_anomaly_detection_brain_mri_amd.gan_engine import GanEngine, ZimmererEngine  # noqa: E402

SURFACE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'engine_surface.json')
# The only differences from the recorded surface that are allowed: parameters with defaults added at the end.
ADDED_DEFAULTS = {'GanEngine.buffer': ('(self, which=0)', '(self, which=0, write=True)'),
                  'ZimmererEngine.buffer': ('(self, which=0)', '(self, which=0, write=True)')}


def _describe(owner, name):
    static = inspect.getattr_static(owner, name)
    if isinstance(static, property):
        return 'property'
    value = getattr(owner, name)
    if callable(value):
        return str(inspect.signature(value))
    return 'attribute'


def surface():
    """{'Engine.forward': '(self, x, ...)', ..., 'engine.rng_fill': '(jobs, ...)'}: every public name of the engine classes (inherited ones
    included) and every public function the two modules define."""
    out = {}
    for cls in (Engine, GanEngine, ZimmererEngine, Scores):
        for name in dir(cls):
            if not name.startswith('_'):
                out[f'{cls.__name__}.{name}'] = _describe(cls, name)
    for mod in (engine, gan_engine):
        short = mod.__name__.rsplit('.', 1)[1]
        for name, value in vars(mod).items():
            if not name.startswith('_') and inspect.isfunction(value) and value.__module__ == mod.__name__:
                out[f'{short}.{name}'] = str(inspect.signature(value))
    return out


def _resolve(key):
    owner, name = key.split('.', 1)
    scope = {'Engine': Engine, 'GanEngine': GanEngine, 'ZimmererEngine': ZimmererEngine, 'Scores': Scores, 'engine': engine,
             'gan_engine': gan_engine}[owner]
    assert hasattr(scope, name), f'{key} is gone'
    return _describe(scope, name) if inspect.isclass(scope) else str(inspect.signature(getattr(scope, name)))


def test_public_surface_is_the_recorded_one():
    with open(SURFACE) as f:
        recorded = json.load(f)
    assert len(recorded) > 150 and 'Engine.resize' in recorded and 'GanEngine.get_grads' in recorded and 'engine.rng_fill' in recorded
    seen = set()
    for key, was in recorded.items():
        now = _resolve(key)
        if key in ADDED_DEFAULTS:
            assert (was, now) == ADDED_DEFAULTS[key], (key, was, now)
            seen.add(key)
        else:
            assert now == was, (key, was, now)
    assert seen == set(ADDED_DEFAULTS)


def test_engines_are_device_ops():
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    for cls in (Engine, GanEngine, ZimmererEngine):
        assert issubclass(cls, DeviceOps)


def test_one_implementation_of_every_op():
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    from unsupervised_anomaly_detection_brain_mri_amd.utils.order_stats import OrderStatOps
    names = sorted(n for c in (DeviceOps, OrderStatOps) for n, v in vars(c).items() if not n.startswith('_') and callable(v))
    assert {'erode_cross', 'zoom', 'rotate', 'resize', 'curvature_flow', 'crop', 'region_props', 'render_heatmap', 'labelled_histogram',
            'scores', 'residual', 'quantile', 'percentile', 'histogram'} <= set(names)
    for name in names:
        if name == 'close':             # DeviceOps.close is the no-op a handle replaces
            continue
        for cls in (Engine, GanEngine):
            assert getattr(cls, name) is getattr(DeviceOps, name), (cls.__name__, name)


def test_device_ops_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from unsupervised_anomaly_detection_brain_mri_amd.device_ops import DeviceOps
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        DeviceOps()


if __name__ == '__main__':
    json.dump(surface(), sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write('\n')
