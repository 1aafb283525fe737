"""Builds the host emulators of tests/native/ (the kernel source of a csrc/*.hip file compiled for the CPU behind tests/native/hip_host_emu.h)
for the tests/test_*_kernels_host.py files."""
import os
import shutil
import subprocess

from unsupervised_anomaly_detection_brain_mri_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def clangxx():
    hipcc = os.environ.get('HIPCC') or shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    for c in (os.path.join(os.path.dirname(os.path.realpath(hipcc)), '..', 'lib', 'llvm', 'bin', 'clang++'), '/opt/rocm/lib/llvm/bin/clang++',
              shutil.which('clang++'), shutil.which('g++')):
        if c and os.path.exists(c):
            return c
    raise RuntimeError('no host C++ compiler found (the HIP toolchain ships clang++)')


def build_emu(tmp_path_factory, name, hip_source):
    """Compiles tests/native/<name>.cpp, which includes csrc/<hip_source>, and returns the executable's path.  The emulator must round as the
    device build of that file does: it gets -ffp-contract=off exactly when build.EXTRA_FLAGS gives it to hip_source."""
    exe = str(tmp_path_factory.mktemp(name) / name)
    contract = [f for f in build.EXTRA_FLAGS.get(hip_source, []) if f == '-ffp-contract=off']
    subprocess.run([clangxx(), '-std=c++20', '-O1', *contract, '-x', 'c++', '-Wno-unknown-pragmas', os.path.join(ROOT, 'tests', 'native', name + '.cpp'),
                    '-o', exe, '-lpthread'], check=True)
    return exe
