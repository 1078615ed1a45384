"""Static wait-state check (tools/hazard_lint.py, rules R1-R7 incl. no packed-fp32 instructions) of the vector-matrix samplers'
position-gradient translation unit, compiled with the library's own flags (build.FLAGS) as tests/test_hazards_vm.py does
for vm.hip."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
sys.path.insert(0, REPO)
from directvoxgo_amd.build import FLAGS as BUILD_FLAGS  # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = [f for f in BUILD_FLAGS if f not in ('-shared', '-Wall', '-Wno-unused-function')] + ['-S', '--cuda-device-only']

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='needs hipcc')


def test_vm_xyz_breaks_no_wait_state_rule(tmp_path):
    import hazard_lint as H
    out = tmp_path / 'vm_xyz.s'
    subprocess.run([HIPCC] + FLAGS + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'vm_xyz.hip'), '-o', str(out)], check=True,
                   capture_output=True)
    bad, names = [], []
    for name, items in H.parse(str(out)).items():
        if not any(k == 'ins' for k, _ in items):
            continue
        names.append(name)
        bad += H.check_kernel(name, items)[0]
    assert sum('vm_bwd_xyz_kernel' in n for n in names) == 4                     # VEC = 4, 1 x features, density
    assert not bad, '\n'.join(bad[:20])
    text = out.read_text()
    assert '_atomic_' not in text                                           # every row is written with plain stores
    assert 'scratch_' not in text                                           # no kernel spills or indexes private memory
