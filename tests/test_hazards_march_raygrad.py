"""The compiler's resource summary of the ray-gradient kernels of the fused march (csrc/march_raygrad.hip: march_ray_bwd_kernel, both
dispatch variants), compiled with the library's own flags (build.FLAGS) as tests/test_hazards_raygrad.py does for the sampler's
position gradient: no private memory, no spilled register.  Reads the kernel descriptors' metadata only; the wait-state rules
of the whole translation unit are tests/test_hazards.py's."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from directvoxgo_amd.build import FLAGS as BUILD_FLAGS, HEADERS, SOURCES  # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = [f for f in BUILD_FLAGS if f not in ('-shared', '-Wall', '-Wno-unused-function')] + ['-S', '--cuda-device-only']

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')


@pytest.fixture(scope='module')
def meta(tmp_path_factory):
    assert 'march_raygrad.hip' in SOURCES and 'xyz_corners.h' in HEADERS
    out = tmp_path_factory.mktemp('march_raygrad') / 'march_raygrad.s'
    subprocess.run([HIPCC] + FLAGS + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'march_raygrad.hip'), '-o', str(out)], check=True,
                   capture_output=True)
    text = out.read_text()
    return text[text.index('amdhsa.kernels:'):]


def test_march_ray_bwd_kernels_use_no_private_memory(meta):
    """one metadata entry per kernel: from its `.agpr_count` (the first key of an entry) to the next one's"""
    entries = meta.split('  - .agpr_count:')[1:]
    found = {}
    for e in entries:
        name = re.findall(r'^\s*\.symbol:\s*(\S+)\.kd\s*$', e, flags=re.M)      # the entry's descriptor symbol
        assert len(name) == 1, name
        if 'march_ray_bwd_kernel' in name[0]:
            found[name[0]] = (int(re.search(r'\.private_segment_fixed_size:\s*(\d+)', e).group(1)),
                              int(re.search(r'\.vgpr_spill_count:\s*(\d+)', e).group(1)),
                              int(re.search(r'\.sgpr_spill_count:\s*(\d+)', e).group(1)))
    assert len(found) == 2 and any('ILi4E' in n for n in found) and any('ILi1E' in n for n in found), sorted(found)
    assert all(v == (0, 0, 0) for v in found.values()), found
