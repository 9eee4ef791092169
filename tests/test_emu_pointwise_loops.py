"""CPU tier: the persistent tile loops of k_pmlp_fwd, k_pblock_fwd, k_pmlp_bwd (and its LIN form) and k_plin_bwd in host
emulation.  Their workgroup caps (2048 / 2048 / 256 / 512) are far above what the emulation finishes, so each runs in a
fresh child process whose environment carries the diagnostic switch that sets the cap to one workgroup (the emulation
build has -DSC_DIAG; each switch is read once per process): nine tiles are then three trips through the loop, the last with
one tile, and a marked tile in the second trip is the whole weight gradient.  The child sets nothing else."""
import os
import subprocess
import sys

import pytest

from engine_runner import emu_lib

HERE = os.path.dirname(os.path.abspath(__file__))
SWITCHES = {"SC_PMLP_FWD_WGS": 4, "SC_PBLOCK_FWD_WGS": 3, "SC_PLIN_BWD_WGS": 10, "SC_PMLP_BWD_WGS": 25}    # cases the child runs


@pytest.fixture(scope="module", autouse=True)
def built():
    emu_lib()                                                # build once here, not in four children at a time


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_one_workgroup_walks_every_tile(switch):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env[switch] = "1"
    res = subprocess.run([sys.executable, os.path.join(HERE, "pointwise_loop_child.py"), switch], env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert res.stdout.strip().splitlines()[-1] == f"ok {SWITCHES[switch]}", res.stdout[-2000:]


def test_without_the_switch_the_caps_hold():
    """the same shapes in this process, no switch set: nine tiles are three workgroups, none loops"""
    import pointwise_reference as pr
    assert not any(os.environ.get(s) for s in SWITCHES)
    lib = emu_lib()
    cfg = pr.with_tiles(dict(chans=(64, 32, 64), gate=1, act=1, xpre=None, gbias=1, sid=212), 9)
    assert pr.mlp_backward_n_wg(lib, cfg) == 3
    assert pr.linear_backward_n_wg(lib, pr.with_tiles(dict(c=64), 9)) == 3
