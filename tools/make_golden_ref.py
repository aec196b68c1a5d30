#!/usr/bin/env python3
"""Build-container tool: the unmodified reference engine's answers (oracle/_ref) for the inputs of
tests/test_oracle_vs_ref.py -- Viterbi matrices / alignments / scores, Forward matrices and sampled
alignments, RNG draws -- recorded so that those tests run without the reference.  The inputs and the
reduction to digests and bits are the test module's own.

    python tools/make_golden_ref.py        # writes tests/golden/oracle_vs_ref.json
"""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import pyoracle as orc  # noqa: E402
from tests import test_oracle_vs_ref as t  # noqa: E402

assert orc.ref_available(), "oracle/_ref is not built (make ref; needs the reference sources)"
orc.lib()


def section(table, cases, live):
    return {"inputs_sha256": t.inputs_digest(table, cases), "cases": [live(*c) for c in cases]}


out = {"source": "oracle/_ref (the unmodified reference engine); tools/make_golden_ref.py",
       "gap_open": float(t.G), "gap_extend": float(t.E), "viterbi": {}, "forward": {}}
for L in (1, 3):
    for kind in ("random", "ties"):
        table, pairs = t.viterbi_inputs(L, kind)
        out["viterbi"][f"L{L}_{kind}"] = section(table, pairs, lambda anc, des: t.ref_viterbi_record(orc, table, L, anc, des))
    table, cases = t.forward_inputs(L)
    out["forward"][f"L{L}"] = section(table, cases, lambda anc, des, seeds: t.ref_forward_record(orc, table, L, anc, des, seeds))
out["rng"] = {"f24": section(np.zeros(0, np.float32), [(s,) for s in t.RNG_SEEDS], lambda s: t.ref_rng_record(orc, s))}
path = ROOT / "tests" / "golden" / "oracle_vs_ref.json"
path.write_text(json.dumps(out, indent=0) + "\n")
print(f"wrote {path.relative_to(ROOT)} ({path.stat().st_size} bytes)")
