"""CPU tier: ``fno_block_precision`` "half" / "mixed" on the mode-parallel layer (gloo world 2 and 4, every local stage on
the host-emulation build of the engine, tests/emu_engine.py), against the single-process ``SpectralConv._forward_half``
on the full batch.  The half route exchanges xhat / yhat / g_yhat / g_xhat on the complex32 wire
(mappings.all_to_all_c32): each is a float16 value where it is read, so the layer computes what one process computes --
every value of y, x.grad and the weight gradients bit for bit (the bar allows the single-GPU half rule: one float16
step, >= 99.9 % identical; gradients rel-L2 <= 1e-5).  The same step at "full" must miss that bar, and it must move
exactly twice the bytes.  Test infrastructure only: the product refuses CPU tensors."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

# (spatial, ctor n_modes, runtime n_modes or None, precision, factorization, bias, samples per rank, Cin, Cout)
CASES = {
    2: [((16, 12), (8, 8), None, "half", None, True, 2, 3, 4),
        ((16, 12), (8, 8), (6, 6), "mixed", None, False, 1, 2, 3),       # reduced n_modes: w0 > 0 on the wire
        ((16, 12), (8, 6), None, "mixed", "tucker", True, 1, 3, 2),
        ((16, 12), (8, 8), (6, 4), "half", "tucker", False, 2, 2, 2),
        ((8, 8, 6), (6, 4, 4), None, "mixed", None, True, 1, 2, 3),      # 3-d
        ((8, 8, 6), (6, 4, 4), (4, 4, 2), "half", None, True, 1, 2, 2)],
    4: [((16, 12), (6, 6), None, "half", None, True, 1, 2, 3),           # 6 rows over 4 ranks of 2: zero rows
        ((8, 6, 8), (6, 4, 6), (4, 4, 4), "mixed", "tucker", False, 1, 2, 2)],
}


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from emu_engine import engine_on_emulation
    from neuraloperator_amd import SpectralConv
    from neuraloperator_amd.mpu import ModeParallelSpectralConv, comm
    from neuraloperator_amd.mpu.mappings import A2A_STATS

    comm.init(model_parallel_size=world, backend="gloo")
    out = {}
    for i, (spatial, modes, run_modes, prec, fac, bias, bl, ci, co) in enumerate(CASES[world]):
        B = bl * world
        torch.manual_seed(i)                                   # identical full tensors and parameters on every rank
        x = torch.randn(B, ci, *spatial)
        kw = dict(factorization=fac, rank=0.6) if fac else {}
        single = SpectralConv(ci, co, modes, bias=bias, fno_block_precision=prec, **kw)
        with torch.no_grad():
            for q in single.parameters():                      # O(1) weights: the half rounding is not lost in noise
                q.copy_(torch.randn_like(q) * (0.7 if fac else 0.5))
        sd = single.state_dict()
        if run_modes is not None:
            single.n_modes = run_modes
        res = {}
        with engine_on_emulation():
            xf = x.clone().requires_grad_(True)
            yf = single._forward_half(xf, list(spatial))
            g = torch.randn(*yf.shape, generator=torch.Generator().manual_seed(100 + i))
            yf.backward(g.to(yf.dtype))
            ref = dict(y=yf.detach()[rank * bl:(rank + 1) * bl].float(), gx=xf.grad[rank * bl:(rank + 1) * bl])
            for p in ("half_or_mixed", "full"):
                layer = ModeParallelSpectralConv(ci, co, modes, bias=bias, fno_block_precision=prec if p != "full" else "full",
                                                 **kw)
                layer.load_full_state_dict(sd)
                if run_modes is not None:
                    layer.n_modes = run_modes
                xs = x[rank * bl:(rank + 1) * bl].clone().requires_grad_(True)
                A2A_STATS["bytes"] = 0
                y = layer(xs)
                y.backward(g[rank * bl:(rank + 1) * bl].to(y.dtype))
                layer.reduce_replicated_grads()
                res[p] = dict(y=y.detach(), dtype=str(y.dtype), gx=xs.grad, bytes=A2A_STATS["bytes"],
                              grads=_grads(layer, single, fac, rank, world, bias))
            with pytest.raises(ValueError):
                ModeParallelSpectralConv(ci, co, modes, fno_block_precision="quarter")
        out[i] = dict(ref=ref, res=res, bias=bias, b=(None if not bias else single.bias.detach()))
    ret[rank] = out
    comm.cleanup()


def _grads(layer, single, fac, rank, world, bias):
    """[(name, this rank's gradient, the single process's gradient of the same entries)]"""
    rows = layer.rows
    k1 = layer.max_n_modes[0]
    live = max(0, min(rows, k1 - rank * rows))
    pairs = []
    if fac is None:
        pairs.append(("w", layer.weight.grad[:, :, :live], single.weight.tensor.grad[:, :, rank * rows:rank * rows + live]))
    else:
        pairs.append(("core", layer.core.grad, single.weight.core.grad))
        for j, f in enumerate(layer.factors):
            fs = single.weight.factors[j].grad
            pairs.append((f"factor{j}", f.grad[:live] if j == 2 else f.grad,
                          fs[rank * rows:rank * rows + live] if j == 2 else fs))
    if bias:
        pairs.append(("bias", layer.bias.grad, single.bias.grad))
    return [(n, a.detach().clone(), b.detach().clone()) for n, a, b in pairs]


def _rel(a, b):
    return float((a - b).abs().pow(2).sum().sqrt() / b.abs().pow(2).sum().sqrt().clamp_min(1e-30))


def meets_half_bar(y, ref, bias):
    """the single-GPU half rule: within one float16 step of the pre-bias value, >= 99.9 % of the elements identical"""
    yb, rb = (y.float() - bias, ref - bias) if bias is not None else (y.float(), ref)
    step = torch.maximum(rb.abs(), torch.tensor(6.1e-5)) * 2.0 ** -10
    within = bool(((yb - rb).abs() <= 1.01 * step).all())
    same = (y.float() == ref).float().mean().item()
    return within and same >= 0.999


@pytest.mark.parametrize("world", [2, 4])
def test_mode_parallel_half_is_the_single_process_half_layer(world):
    from engine_runner import emu_lib
    from neuraloperator_amd.mpu import comm
    emu_lib()                                   # build the emulation library once, before the workers race for it
    port = comm.free_port()
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    procs = [ctx.Process(target=_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(900)
        assert p.exitcode == 0, f"worker exit code {p.exitcode}"
    for r in range(world):
        for i, case in ret[r].items():
            tag = (world, r, CASES[world][i])
            ref, half, full = case["ref"], case["res"]["half_or_mixed"], case["res"]["full"]
            assert half["dtype"] == ("torch.float32" if case["bias"] else "torch.float16"), tag
            assert meets_half_bar(half["y"], ref["y"], case["b"]), tag
            assert _rel(half["gx"], ref["gx"]) <= 1e-5, (tag, _rel(half["gx"], ref["gx"]))
            for name, a, b in half["grads"]:
                assert _rel(a, b) <= 1e-5, (tag, name, _rel(a, b))
            # the fp32 layer computes something else: the test sees the feature
            assert not meets_half_bar(full["y"], ref["y"], case["b"]), tag
            # four exchanges on the complex32 wire: exactly half the bytes of the fp32 wire
            assert half["bytes"] > 0 and 2 * half["bytes"] == full["bytes"], (tag, half["bytes"], full["bytes"])
