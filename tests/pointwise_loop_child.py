"""Child process of tests/test_emu_pointwise_loops.py: one grid switch of the emulation build (read once per process, so
set in this process's environment by the parent) makes one workgroup walk all tiles of a pass.  Runs T = 9 (B = 3, S = 96:
three rounds of four waves, the last with one tile) and, for the backward passes, T = 5 and 9 with gout zero outside one
tile, against the float64 helper of tests/pointwise_reference.py.  Prints one line per case and `ok <n>` at the end."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import pointwise_reference as pr  # noqa: E402
from engine_runner import emu_lib  # noqa: E402

MLP_BWD = [dict(chans=pr.MLP_SHAPES[sid], gate=1, act=1, xpre=xp, gbias=1, sid=sid) for sid, xp in ((111, "grad"), (212, "pre"), (222, None))]
BLOCK_BWD = [dict(chans=pr.MLP_SHAPES[sid][:2], act=act, sid=sid) for sid, act in ((111, pr.ACT_GELU), (212, pr.ACT_DGRAD))]
CASES = {
    "SC_PMLP_FWD_WGS": [("mlp_fwd", dict(chans=ch, gate=1, act=1, bias=1, sid=sid)) for sid, ch in pr.MLP_SHAPES.items()],
    "SC_PBLOCK_FWD_WGS": [("block_fwd", dict(chans=pr.MLP_SHAPES[sid][:2], act=pr.ACT_DGRAD, bias=1, sid=sid)) for sid in (111, 212, 222)],
    "SC_PLIN_BWD_WGS": [("lin_bwd", dict(c=c, addend=1, gbias=1)) for c in (32, 64)],
    "SC_PMLP_BWD_WGS": [("mlp_bwd", c) for c in MLP_BWD] + [("block_bwd", c) for c in BLOCK_BWD],
}


def main(switch):
    assert os.environ.get(switch) == "1", "the parent sets the switch"
    lib, n = emu_lib(), 0
    for kind, cfg in CASES[switch]:
        backward = kind.endswith("bwd")
        nine = pr.with_tiles(cfg, 9)
        pr.run_case(kind, lib, nine, seed=3, guard=True, expect_n_wg=1 if backward else None)
        n += 1
        if backward:                                         # R = 4: tile 4 opens the second round, tile 3 closes the first
            for cfg_t, tile in ((pr.with_tiles(cfg, 5), 4), (pr.with_tiles(cfg, 5), 0), (pr.with_tiles(cfg, 5), 3), (nine, 8)):
                got, _, _ = pr.run_case(kind, lib, cfg_t, seed=3, mark=tile, expect_n_wg=1)
                pr.assert_zero_outside_tile(got, cfg_t, tile)
                n += 1
    print("ok", n)


if __name__ == "__main__":
    main(sys.argv[1])
