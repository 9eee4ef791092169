"""Recorder of tests/golden/attn_*.npz -- run by hand where the reference exists:

    python tests/record_attention.py

Loads the verbatim ``neuralop/layers/attention_kernel_integral.py`` and ``neuralop/layers/embeddings.py`` by path, builds
AttentionKernelIntegral under the case's seed in fp32 (the state dict of the record), copies it to float64 and runs it on
the fp32-representable inputs of attention_reference.case_inputs with the cotangent g.  Each file holds the inputs,
positions, weights and g, the state dict ("state:<key>"), the float64 ``out`` and every gradient ("grad:u_src",
"grad:u_qry", "grad:<parameter>"), for the cases that ask for it the kernel matrix of the non-associative form, and under
"err:<tensor>" the rel-L2 error of the verbatim fp32 module against that float64 run; each stays under 200 KB (for
that the results of a "compact" case are stored rounded to fp32, its gradients in attn_<case>.grads.npz).
Cases: attention_reference.CASES."""
import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import attention_reference as ar  # noqa: E402
import ref_verbatim  # noqa: E402


def load(name, filename):
    path = os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "layers", filename)
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_classes():
    return (load("_ref_attention_kernel_integral", "attention_kernel_integral.py").AttentionKernelIntegral,
            load("_ref_embeddings", "embeddings.py").RotaryEmbedding2D)


def run(m, emb, t, cfg, dtype):
    t = {k: v.to(dtype) for k, v in t.items()}
    for k in ("u_src", "u_qry"):
        if k in t:
            t[k] = t[k].clone().requires_grad_(True)
    out = ar.call_layer(m, emb, t)
    out.backward(t["g"])
    res = {"out": out.detach()}
    res.update({"grad:" + k: v for k, v in ar.grads_of(m, t).items()})
    if cfg["kernel"]:
        with torch.no_grad():
            res["kernel"] = ar.call_layer(m, emb, t, associative=False, return_kernel=True)[1]
    return res


def record(name, cfg, seed, classes):
    cls, emb_cls = classes
    m32, emb32 = ar.build_layer(cls, emb_cls, cfg, seed)
    state = {k: v.detach().clone() for k, v in m32.state_dict().items()}
    t = ar.case_inputs(cfg, seed)
    m64, emb64 = ar.build_layer(cls, emb_cls, cfg, seed)
    m64.load_state_dict(state)
    m64 = m64.double()
    emb64 = None if emb64 is None else emb64.double()
    want = run(m64, emb64, t, cfg, torch.float64)
    got = run(m32, emb32, t, cfg, torch.float32)
    rec = {k: v.numpy() for k, v in t.items()}
    rec.update({"state:" + k: v.numpy() for k, v in state.items()})
    rec["state_keys"] = np.array(list(state))
    rec["seed"] = np.int64(seed)
    worst = 0.0
    for k, v in want.items():
        # "compact": the float64 result rounded to fp32 (a relative 6e-8 at the most, two orders below the bar), where
        # the parameters of the case alone would take the file past its size limit in float64
        rec[k] = v.numpy().astype(np.float32) if cfg["compact"] else v.numpy()
        rec["err:" + k] = np.float64(ar.rel_l2(got[k].numpy(), v.numpy()))
        worst = max(worst, float(rec["err:" + k]))
    files = {ar.golden_path(name): rec}
    if cfg["compact"]:                                       # the gradients in a file of their own
        files = {ar.golden_path(name): {k: v for k, v in rec.items() if not k.startswith("grad:")},
                 ar.golden_path(name + ".grads"): {k: v for k, v in rec.items() if k.startswith("grad:")}}
    size = 0
    for path, part in files.items():
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 200 * 1024, (path, os.path.getsize(path))
        size += os.path.getsize(path)
    print(f"{name}: {size / 1024:.0f} KB, worst fp32-reference error {worst:.2e} "
          f"(out {float(rec['err:out']):.2e})")
    return worst


def main():
    warnings.filterwarnings("ignore", message="input's size at dim=1 does not match num_features")
    classes = reference_classes()
    worst = max(record(name, cfg, ar.SEEDS[name], classes) for name, cfg in sorted(ar.CASES.items()))
    print(f"worst fp32-reference error over all cases and tensors: {worst:.2e}")


if __name__ == "__main__":
    main()
