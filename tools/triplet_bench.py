#!/usr/bin/env python3
"""Throughput of the triplet-model aligner (coati_hip_triplet_align, csrc/viterbi_tri.hip): GCUPS for N x 1 kb pairs
per model (default 10 000), one model per child process, each child under `timeout -k 10`.  Prints one JSON line per
model and the OpenFst baseline recorded by tools/make_golden_triplet.py (tests/golden/triplet_cases.json: the
reference's FST path per pair, process start included).

    python tools/triplet_bench.py [--pairs 10000] [--codons 333] [--models tri-mg,tri-ecm,dna] [--timeout 900]
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def pairs(n: int, n_codons: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    sense = np.array([c for c in range(64) if c not in (48, 50, 56)])
    lut = np.array([ord(x) for x in "ACGT"], np.uint8)
    out = []
    for _ in range(n):
        c = rng.choice(sense, n_codons)
        anc = np.stack([lut[c >> 4], lut[(c >> 2) & 3], lut[c & 3]], 1).reshape(-1)
        des = anc.copy()
        hit = rng.random(des.size) < 0.05
        des[hit] = lut[rng.integers(0, 4, hit.sum())]
        keep = rng.random(des.size) > 0.01
        out.append((anc.tobytes().decode(), des[keep].tobytes().decode()))
    return out


def child(model: str, n: int, n_codons: int) -> None:
    from coati_amd import hip, host

    cost, pi, _ = host.triplet_model(model)
    m = hip.TripletModel(cost, pi=pi)
    m.align(*hip.triplet_encode(pairs(8, n_codons, seed=1)))  # runtime, code object, first allocation
    enc = hip.triplet_encode(pairs(n, n_codons))
    cells = int(sum((int(enc[1][p + 1] - enc[1][p])) * int(enc[3][p + 1] - enc[3][p]) for p in range(n)))
    t = time.perf_counter()
    sc, *_ = m.align(*enc)
    dt = time.perf_counter() - t
    m.close()
    assert np.isfinite(sc).all()
    print(json.dumps({"model": model, "pairs": n, "len_a": 3 * n_codons, "seconds": round(dt, 4), "cells": cells,
                      "gcups": round(cells / dt / 1e9, 3)}))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--codons", type=int, default=333)
    ap.add_argument("--models", default="tri-mg,tri-ecm,dna")
    ap.add_argument("--timeout", type=int, default=900)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.pairs, args.codons)
        return
    gold = json.loads((ROOT / "tests/golden/triplet_cases.json").read_text())
    for model in args.models.split(","):
        r = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--child", model, "--pairs",
                            str(args.pairs), "--codons", str(args.codons)], capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout + r.stderr, file=sys.stderr)
            sys.exit(r.returncode)
        line = json.loads(r.stdout.strip().splitlines()[-1])
        base = gold["openfst_time"][model]
        line["openfst_ms_per_pair"] = round(base["seconds"] / base["pairs"] * 1e3, 1)
        line["openfst_mcups"] = round(base["cells"] / base["seconds"] / 1e6, 3)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
