"""Static wait-state check (tools/hazard_lint.py, rules R1-R7 incl. no packed-fp32 instructions) of the unbounded-scene
unit (contracted sampler, distortion loss), compiled with the library's own flags (build.FLAGS) as tests/test_hazards.py
does for the other units."""
import os
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


def test_contract_is_built():
    assert 'contract.hip' in SOURCES


def test_contract_breaks_no_wait_state_rule(tmp_path):
    import hazard_lint as H
    out = tmp_path / 'contract.s'
    subprocess.run([HIPCC] + FLAGS + [os.path.join(REPO, 'directvoxgo_amd', 'csrc', 'contract.hip'), '-o', str(out)], check=True,
                   capture_output=True)
    bad, names = [], []
    for name, items in H.parse(str(out)).items():
        if not any(k == 'ins' for k, _ in items):
            continue
        names.append(name)
        bad += H.check_kernel(name, items)[0]
    assert sum('contract_sample_kernel' in n for n in names) == 2, names      # count and emit passes
    assert any('distortion_kernel' in n for n in names), names
    assert not bad, '\n'.join(bad[:20])
