"""viterbi_ck's transposed fills (COATI_HIP_OPT_CK_ORIENT): every score bit and every op byte must be what the
untransposed fill (orientation 0, pinned to the reference by the other GPU tests) computes, under the automatic rule (1)
and with every pair that can be transposed (2)."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
OPT_CK_ORIENT = 4


@pytest.fixture(autouse=True)
def _ck_full_width(monkeypatch):
    """viterbi_ck with 16-column strips whatever the batch size: the planner would give the small batches here to
    viterbi_l1 / viterbi_lp or narrow strips, and transposes only what is one full-width strip transposed."""
    from coati_amd import hip

    monkeypatch.setenv("COATI_HIP_VITERBI_CK", "1")
    monkeypatch.setenv("COATI_HIP_STRIP_W", "16")
    hip.reload_env()
    yield
    monkeypatch.undo()
    hip.reload_env()


def _run(model, packed, orient):
    """One resident batch with the orientation setting in force when it is planned: (scores, [ops per pair], band stats)."""
    from coati_amd import hip

    model.set_option(OPT_CK_ORIENT, orient)
    bt = hip.Batch(model, *packed)
    try:
        bt.viterbi_launch()
        bt.sync()
        scores, ops, off, ln = bt.viterbi_fetch()
        stats = bt.band_stats()
    finally:
        bt.close()
    return scores, [bytes(ops[int(off[p]):int(off[p]) + int(ln[p])]) for p in range(len(scores))], stats


def _same(a, b, what):
    sa, oa, _ = a
    sb, ob, _ = b
    assert np.array_equal(sa.view(np.uint32), sb.view(np.uint32)), what
    bad = [p for p in range(len(oa)) if oa[p] != ob[p]]
    assert not bad, f"{what}: ops differ in {len(bad)} pairs, first {bad[:5]}"


def _all_orientations(model, packed, what):
    r = [_run(model, packed, o) for o in (0, 1, 2)]
    _same(r[0], r[1], f"{what}: auto")
    _same(r[0], r[2], f"{what}: all")
    return r


def test_orient_golden_gap_len_1():
    """The gap-len-1 golden cases (doctests among them) under the three settings, and against the reference's record."""
    from coati_amd import hip, host

    doc = json.loads((GOLD / "viterbi_cases.json").read_text())
    table = np.load(GOLD / "table_mg94_goldenP.npy")
    cases = [c for c in doc["cases"] if c["gap_len"] == 1]
    model = hip.Model(table, host.gap_consts(doc["gap_open"], doc["gap_extend"]), 1)
    r = _all_orientations(model, hip.pack_pairs([host.encode(c["anc"], c["des"]) for c in cases]), "golden")
    for res in r:
        for p, c in enumerate(cases):
            assert int(np.float32(res[0][p]).view(np.uint32)) == int(c["score_bits"], 16), c["name"]
    model.close()


def _synthetic(rng, n, kind):
    pairs = []
    for _ in range(n):
        anc = util.random_anc(rng, 334)  # 1 002 nt, as in the benchmark
        des = util.mutate(rng, anc, sub=0.08, n_indel=2)
        if kind == "long":  # lb > 1 024: two strips untransposed, one transposed
            des = des + util.random_anc(rng, int(rng.integers(10, 30)))
        elif kind == "short":  # lb < la
            des = des[: len(des) - int(rng.integers(3, 80))]
        elif kind == "equal":
            des = util.mutate(rng, anc, sub=0.08, n_indel=0)
        elif kind == "bigindel":  # a 90-300 nt deletion early and an insertion as long later: the path leaves the band
            ln = int(rng.integers(90, 301))  # (the band widens with the length difference, which this keeps at ~0)
            pos = int(rng.integers(0, 300))
            des = des[:pos] + des[pos + ln:]
            pos = int(rng.integers(len(des) - 300, len(des)))
            des = des[:pos] + util.random_anc(rng, ln // 3 + 1)[:ln] + des[pos:]
        pairs.append((util.encode_anc(anc), util.encode_des(des)))
    return pairs


@pytest.mark.parametrize("kind", ["long", "short", "equal"])
def test_orient_synthetic_shapes(kind):
    from coati_amd import hip, host

    rng = np.random.default_rng({"long": 1, "short": 2, "equal": 3}[kind])
    pairs = _synthetic(rng, 96, kind)
    model = hip.Model(host.set_subst("mar-mg"), host.gap_consts(), 1)
    _all_orientations(model, hip.pack_pairs(pairs), kind)
    model.close()


def test_orient_tie_table():
    from coati_amd import hip, host

    rng = np.random.default_rng(4)
    pairs = _synthetic(rng, 48, "long") + _synthetic(rng, 48, "short") + util.encode_pairs(util.make_pairs(rng, 64, min_cod=1, max_cod=120))
    model = hip.Model(util.tie_table(), host.gap_consts(), 1)
    _all_orientations(model, hip.pack_pairs(pairs), "ties")
    model.close()


def test_orient_band_refills_in_transposed_pairs():
    """Pairs with a long indel leave the kept band; under setting 2 every pair is transposed, so the refills counted there
    are refills of transposed pairs, and their results must still be the untransposed ones."""
    from coati_amd import hip, host

    rng = np.random.default_rng(5)
    pairs = _synthetic(rng, 128, "bigindel")
    model = hip.Model(host.set_subst("mar-mg"), host.gap_consts(), 1)
    r = _all_orientations(model, hip.pack_pairs(pairs), "big indels")
    band, twice = r[2][2]
    assert band > 0 and twice > 0, r[2][2]
    model.close()


def test_orient_full_workload():
    """The benchmark's 10 000 pairs -- cut pairs and walk items among them -- byte for byte under the three settings."""
    from coati_amd import hip, host

    model = hip.Model(host.set_subst("mar-mg"), host.gap_consts(), 1)
    _all_orientations(model, host.synth_encoded(0, 10000), "10 000 pairs")
    model.close()


def test_orient_streamed_call_unchanged():
    """A streamed coati_hip_viterbi_batch call (never transposed) computes what a transposing resident batch does."""
    from coati_amd import hip, host

    packed = host.synth_encoded(0, 3000)
    model = hip.Model(host.set_subst("mar-mg"), host.gap_consts(), 1)
    scores, ops, off, ln = model.viterbi(*packed)
    res = _run(model, packed, 1)
    _same((scores, [bytes(ops[int(off[p]):int(off[p]) + int(ln[p])]) for p in range(len(scores))], None), res, "streamed")
    model.close()
