"""Static wait-state check (tools/hazard_lint.py, rules R1-R7 incl. no packed-fp32 instructions) of the position-gradient
sampler's translation unit, compiled with the library's own flags (build.FLAGS) as tests/test_hazards_triplane.py does for
the tri-plane sampler; and the compiler's resource summary of its kernels: both dispatch variants, no private memory."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, REPO)
from directvoxgo_amd.build import FLAGS as BUILD_FLAGS, SOURCES  # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = [f for f in BUILD_FLAGS if f not in ('-shared', '-Wall', '-Wno-unused-function')] + ['-S', '--cuda-device-only']

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')


@pytest.fixture(scope='module')
def asm(tmp_path_factory):
    assert 'grid_sample_xyz.hip' in SOURCES
    out = tmp_path_factory.mktemp('raygrad') / 'grid_sample_xyz.s'
    subprocess.run([HIPCC] + FLAGS + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'grid_sample_xyz.hip'), '-o', str(out)], check=True,
                   capture_output=True)
    return out


def test_raygrad_breaks_no_wait_state_rule(asm):
    import hazard_lint as H
    bad, names = [], []
    for name, items in H.parse(str(asm)).items():
        if not any(k == 'ins' for k, _ in items):
            continue
        names.append(name)
        bad += H.check_kernel(name, items)[0]
    kernels = [n for n in names if 'grid_sample_bwd_xyz_kernel' in n]
    assert len(kernels) == 2 and any('ILi4E' in n for n in kernels) and any('ILi1E' in n for n in kernels), names
    assert not bad, '\n'.join(bad[:20])


def test_raygrad_kernels_use_no_private_memory(asm):
    """the kernel descriptors' metadata (what the loader allocates per lane), not the instruction text"""
    text = asm.read_text()
    meta = text[text.index('amdhsa.kernels:'):]
    names = re.findall(r'^\s*\.name:\s*(\S+)', meta, flags=re.M)
    private = [int(v) for v in re.findall(r'^\s*\.private_segment_fixed_size:\s*(\d+)', meta, flags=re.M)]
    spills = [int(v) for v in re.findall(r'^\s*\.vgpr_spill_count:\s*(\d+)', meta, flags=re.M)]
    kernels = [n for n in names if 'grid_sample_bwd_xyz_kernel' in n]
    assert len(kernels) == 2 and len(private) == len(kernels) == len(spills)
    assert private == [0, 0] and spills == [0, 0]
