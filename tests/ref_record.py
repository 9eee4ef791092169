"""TEST INFRASTRUCTURE: what the verbatim reference returned, recorded under tests/golden/ so that a test compares
against it where the reference tree does not exist (the GPU box, a clean checkout).

``expected(fixture, key, compute)``: ``compute(ref)`` turns the reference's results for one test case into plain JSON
values -- tensor digests (``digest``: dtype, shape and sha256 of the bytes, i.e. bit equality), shapes, flags.  Where
the reference exists the record is computed live and must equal the stored one; ``SC_RECORD_REFERENCE=1`` (one pytest
process: ``SC_TEST_WORKERS=0``) stores it instead.  Without the reference the stored record is returned.  Inputs come
from ``seeded_randn`` (a CPU generator seeded from the case key), so that both sides see the same values."""
import hashlib
import json
import os
import zlib

import torch

from oracle import ref_verbatim

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_CACHE = {}


def digest(t):
    t = t.detach().contiguous().cpu()
    return f"{str(t.dtype)[6:]}{list(t.shape)}:" + hashlib.sha256(t.numpy().tobytes()).hexdigest()[:32]


def seeded_randn(key, *shape):
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    return torch.randn(*shape, generator=g)


def _path(fixture):
    return os.path.join(GOLDEN_DIR, fixture + ".json")


def _stored(fixture):
    if fixture not in _CACHE:
        p = _path(fixture)
        _CACHE[fixture] = json.load(open(p)) if os.path.isfile(p) else {}
    return _CACHE[fixture]


def expected(fixture, key, compute, load=ref_verbatim.load_reference):
    stored = _stored(fixture)
    if not ref_verbatim.available():
        assert key in stored, f"no reference record {key!r} in tests/golden/{fixture}.json"
        return stored[key]
    live = json.loads(json.dumps(compute(load())))
    if os.environ.get("SC_RECORD_REFERENCE") == "1":
        stored[key] = live
        with open(_path(fixture), "w") as f:
            json.dump(stored, f, indent=0, sort_keys=True)
            f.write("\n")
    else:
        assert stored.get(key) == live, f"tests/golden/{fixture}.json[{key!r}] is not what the reference returns"
    return live
