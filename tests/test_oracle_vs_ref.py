"""Pin the CPU oracle bit-for-bit against the unmodified reference DP engine
(src/lib/align_pair.cc compiled into oracle/_ref by `make -C oracle ref`).

The reference's answers for these inputs are recorded in tests/golden/oracle_vs_ref.json
(tools/make_golden_ref.py): DP matrices as SHA-256 digests of their fp32 bits, alignments as
strings, scores and random draws as fp32 bits.  Every test checks the oracle against that record;
where oracle/_ref is built it also recomputes the record with the reference and requires it to be
the stored one."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from tests import util

GOLD = Path(__file__).resolve().parent / "golden"
G, E = np.float32(0.001), np.float32(1.0) - np.float32(1.0) / np.float32(6.0)
N_SAMPLES = 12
RNG_SEEDS = (["42"], [""], ["random42"], ["1", "2", "abc"], ["-17"], ["2147483648"], ["0042"], ["+5"])
RNG_DRAWS = 32


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def digest(*arrays):
    """SHA-256 over the shapes and fp32 bits of `arrays`: equal digests <=> bit-identical arrays."""
    h = hashlib.sha256()
    for x in arrays:
        x = np.ascontiguousarray(x, np.float32)
        h.update(repr(x.shape).encode())
        h.update(x.view(np.uint32).tobytes())
    return h.hexdigest()


# ---- the inputs (shared with tools/make_golden_ref.py) -----------------------------------------------------
def viterbi_inputs(L, table_kind):
    rng = np.random.default_rng(100 + L)
    table = util.random_table(rng) if table_kind == "random" else util.tie_table()
    pairs = util.make_pairs(rng, 60, 0, 40, L=L, amb=0.05) + [("", ""), ("AAA" * L, ""), ("", "ACG" * L)]
    return table, pairs


def forward_inputs(L):
    rng = np.random.default_rng(200 + L)
    table = util.random_table(rng)
    pairs = util.make_pairs(rng, 30, 0, 25, L=L) + [("", "")]
    return table, [(anc, des, ["42"] if k % 2 else [f"s{k}", "7"]) for k, (anc, des) in enumerate(pairs)]


def inputs_digest(table, cases):
    """Ties a record to the inputs it was made from (the generators above run on numpy's seeded streams)."""
    return hashlib.sha256(digest(table).encode() + json.dumps(cases).encode()).hexdigest()


# ---- the reference's answers, reduced to what is recorded ---------------------------------------------------
def ref_viterbi_record(oracle, table, L, anc, des):
    M, D, I, sa, sb, sc = oracle.ref_viterbi(table, G, E, L, anc, des, util.encode_anc(anc), util.encode_des(des))
    return {"mdi_sha256": digest(M, D, I), "aligned": [sa, sb], "score_bits": int(bits(sc))}


def ref_forward_record(oracle, table, L, anc, des, seeds):
    mats, alns, scores = oracle.ref_forward_sample(table, G, E, L, anc, des, util.encode_anc(anc), util.encode_des(des),
                                                   seeds, N_SAMPLES)
    return {"mats_sha256": digest(mats), "aligned": [[sa, sb] for sa, sb in alns], "score_bits": bits(scores).tolist()}


def ref_rng_record(oracle, seeds):
    return bits(oracle.ref_rng_f24(seeds, RNG_DRAWS)).tolist()


def reference(oracle, section, key, table, cases, live):
    """The recorded answers for `cases` (the inputs must be the recorded ones); where the reference is built, its
    answers computed now by live(*case) must equal them."""
    rec = json.loads((GOLD / "oracle_vs_ref.json").read_text())[section][key]
    assert rec["inputs_sha256"] == inputs_digest(table, cases), f"{section}/{key}: inputs differ from the recorded ones"
    if oracle.ref_available():
        assert [live(*c) for c in cases] == rec["cases"], f"{section}/{key}: the reference disagrees with the record"
    return rec["cases"]


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("table_kind", ["random", "ties"])
def test_viterbi_matrices_alignment_score(oracle, L, table_kind):
    table, pairs = viterbi_inputs(L, table_kind)
    want = reference(oracle, "viterbi", f"L{L}_{table_kind}", table, pairs,
                     lambda anc, des: ref_viterbi_record(oracle, table, L, anc, des))
    consts = oracle.gap_consts(G, E)
    for (anc, des), rec in zip(pairs, want):
        a, b = util.encode_anc(anc), util.encode_des(des)
        Mo, Do, Io = oracle.fill(oracle.TROPICAL, table, consts, L, a, b)
        assert digest(Mo, Do, Io) == rec["mdi_sha256"], (anc, des)
        ops, score = oracle.traceback(Mo, Do, Io, consts, L)
        assert list(oracle.ops_to_strings(ops, anc, des)) == rec["aligned"]
        assert int(bits(score)) == rec["score_bits"]
        ops2, score2 = oracle.viterbi(table, consts, L, a, b, lowmem=True)
        assert (ops2 == ops).all() and bits(score2) == bits(score)


@pytest.mark.parametrize("L", [1, 3])
def test_forward_and_sampleback(oracle, L):
    table, cases = forward_inputs(L)
    want = reference(oracle, "forward", f"L{L}", table, cases,
                     lambda anc, des, seeds: ref_forward_record(oracle, table, L, anc, des, seeds))
    consts = oracle.gap_consts(G, E)
    for (anc, des, seeds), rec in zip(cases, want):
        a, b = util.encode_anc(anc), util.encode_des(des)
        M, D, I, Ed = oracle.fill(oracle.LOG, table, consts, L, a, b, edges=True)
        mine = np.concatenate([np.stack([M, D, I]), Ed])
        assert digest(mine) == rec["mats_sha256"], (anc, des)
        r1, r2 = oracle.rng_seed(seeds), oracle.rng_seed(seeds)
        assert len(rec["aligned"]) == len(rec["score_bits"]) == N_SAMPLES
        for aligned, sc in zip(rec["aligned"], rec["score_bits"]):
            ops, s1 = oracle.sampleback(mine, L, r1)
            assert list(oracle.ops_to_strings(ops, anc, des)) == aligned
            assert int(bits(s1)) == sc
            ops2, s2 = oracle.sampleback_mdi(M, D, I, table, consts, L, a, b, r2)
            assert (ops2 == ops).all() and bits(s2) == bits(s1)
            assert bits(oracle.path_logweight(M, D, I, table, consts, L, a, b, ops)) == bits(s1)


def test_rng_stream(oracle):
    cases = [(seeds,) for seeds in RNG_SEEDS]
    want = reference(oracle, "rng", "f24", np.zeros(0, np.float32), cases, lambda seeds: ref_rng_record(oracle, seeds))
    for (seeds,), rec in zip(cases, want):
        r = oracle.rng_seed(seeds)
        got = np.array([oracle.rng_f24(r) for _ in range(RNG_DRAWS)], np.float32)
        assert bits(got).tolist() == rec, seeds
