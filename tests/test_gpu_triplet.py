"""Triplet models (tri-mg, tri-ecm, dna) on the GPU (csrc/viterbi_tri.hip through coati_hip_triplet_align), against
the reference's FST aligner: its doctest outputs (align_fst.cc TEST_CASE "fst_alignment") and the answers recorded
from its own FST builders and OpenFst in tests/golden/triplet_cases.json (tools/make_golden_triplet.py).

Scores: OpenFst's Determinize merges subsets whose residual weights agree within kDelta = 1/1024 (fst/weight.h), so
the reference's distances carry errors of that order -- up to 8.3e-3 (1.2e-3 relative) over the fixtures against the
float64 DP of tests/triplet_dp.py.  The GPU's fp32 scores are compared with the float64 DP tightly and with OpenFst
within FST_TOL.  Alignments: equal to OpenFst's, or a tie -- the GPU alignment's float64 weight equals the optimum."""
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from coati_amd import hip

from tests import triplet_dp as T

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
BIN = ROOT / "coati_amd" / "_build"
GOLD = json.loads((ROOT / "tests" / "golden" / "triplet_cases.json").read_text())
FST_TOL = 2.5e-3     # |GPU - OpenFst| <= FST_TOL * max(1, |score|)
DP_TOL = 2e-5        # |GPU fp32 - float64 DP| <= DP_TOL * max(1, |score|) (fp32 sums of hundreds of path weights)
DOC = ">1\nCTCTGGATAGTG\n>2\nCTATAGTG\n"


def run(*args, timeout=300):
    return subprocess.run([str(BIN / "coati-alignpair"), *map(str, args)], capture_output=True, text=True, timeout=timeout)


def weights(c):
    return T.Weights(c["model"], c["br_len"], c["omega"], c["pi"], c["sigma"], c["gap_open"], c["gap_extend"], c["bc_error"])


def model_of(c):
    from coati_amd import host

    cost, pi, _ = host.triplet_model(c["model"], c["br_len"], c["omega"], c["pi"], c["sigma"])
    return hip.TripletModel(cost, c["gap_open"], c["gap_extend"], pi, c["bc_error"])


@pytest.fixture(scope="module", autouse=True)
def need_device():
    if hip.device_count() == 0:
        pytest.fail("no gfx950 device visible")


# ---- the reference's doctests, byte for byte (the score within FST_TOL: see the module docstring) ----

def check_json(text, want_score):
    m = re.fullmatch(r'\{\n  "alignment": \{\n    "1": "CTCTGGATAGTG",\n    "2": "CT----ATAGTG"\n  \},\n  "score": ([0-9.e+-]+)\n\}\n', text)
    assert m, text
    got = float(m.group(1))
    assert abs(got - want_score) <= FST_TOL * want_score, (got, want_score)
    return got


@pytest.mark.parametrize("model", ["tri-mg", "tri-ecm", "dna"])
def test_doctest_outputs(tmp_path, model):
    fa = tmp_path / "test-fst.fasta"
    fa.write_text(DOC)
    r = run(fa, "-m", model, "-o", tmp_path / "a.json")
    assert r.returncode == 0, r.stderr
    fst = {c["model"]: c["fst_score"] for c in GOLD["cases"] if c["name"].startswith("doctest_fst_alignment")}
    got = check_json((tmp_path / "a.json").read_text(), 9.316000938415527 if model == "tri-mg" else fst[model])
    dp = T.score("CTCTGGATAGTG", "CTATAGTG", T.Weights(model))
    assert abs(got - dp) <= DP_TOL * max(1.0, dp), (got, dp)
    r = run(fa, "-m", model, "-o", tmp_path / "a.phy")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a.phy").read_text().split() == ["2", "12", "1", "CTCTGGATAGTG", "2", "CT----ATAGTG"]
    r = run(fa, "-m", model, "-o", tmp_path / "a.fasta")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "a.fasta").read_text() == ">1\nCTCTGGATAGTG\n>2\nCT----ATAGTG\n"


def test_doctest_end_stop(tmp_path):
    fa = tmp_path / "test-fst.fasta"
    fa.write_text(">1\nCTCTGGATATAA\n>2\nCTATAGTG\n")
    r = run(fa, "-m", "tri-ecm", "-o", tmp_path / "s.fasta")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "s.fasta").read_text() == ">1\nCTCTGGATA---TAA\n>2\nCT----ATAGTG---\n"


def test_stdout_json_default_and_coati_verb(tmp_path):
    fa = tmp_path / "in.fasta"
    fa.write_text(DOC)
    a = run(fa, "-m", "tri-mg")
    b = subprocess.run([str(BIN / "coati"), "alignpair", str(fa), "-m", "tri-mg"], capture_output=True, text=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout
    check_json(a.stdout, 9.316000938415527)


# ---- every fixture through the C ABI, batched and one at a time ----

def groups():
    g = {}
    for c in GOLD["cases"]:
        key = json.dumps({k: c[k] for k in ("model", "br_len", "omega", "pi", "sigma", "gap_open", "gap_extend", "bc_error")})
        g.setdefault(key, []).append(c)
    return list(g.values())


def test_fixtures_batched_and_single():
    worst_fst, worst_dp, ties, n = 0.0, 0.0, 0, 0
    for cases in groups():
        m = model_of(cases[0])
        w = weights(cases[0])
        pairs = [(c["anc_trimmed"], c["des_trimmed"]) for c in cases]
        sc, ops, off, ln = m.align(*hip.triplet_encode(pairs))
        for i, c in enumerate(cases):
            s1, ops1, off1, ln1 = m.align(*hip.triplet_encode([pairs[i]]))
            got = ops[int(off[i]):int(off[i]) + int(ln[i])]
            one = ops1[int(off1[0]):int(off1[0]) + int(ln1[0])]
            assert np.float32(s1[0]).view(np.uint32) == np.float32(sc[i]).view(np.uint32), c["name"]
            assert np.array_equal(got, one), c["name"]
            a, b = T.ops_to_strings(got, *pairs[i])
            dp = T.score(*pairs[i], w)
            scale = max(1.0, abs(dp))
            re64 = T.rescore(*pairs[i], a, b, w)  # the GPU alignment is optimal in float64 ...
            assert abs(re64 - dp) <= 1e-9 * scale, (c["name"], re64, dp)
            assert abs(float(sc[i]) - dp) <= DP_TOL * scale, (c["name"], sc[i], dp)  # ... its fp32 score close to it
            assert abs(float(sc[i]) - c["fst_score"]) <= FST_TOL * scale, (c["name"], sc[i], c["fst_score"])
            if (a, b) != (c["fst_anc"], c["fst_des"]):
                ties += 1  # a tie: the fixture's alignment has the same float64 weight
                assert abs(T.rescore(*pairs[i], c["fst_anc"], c["fst_des"], w) - dp) <= 1e-9 * scale, c["name"]
            worst_fst = max(worst_fst, abs(float(sc[i]) - c["fst_score"]) / scale)
            worst_dp = max(worst_dp, abs(float(sc[i]) - dp) / scale)
            n += 1
        m.close()
    assert n == len(GOLD["cases"])
    print(f"\n{n} fixtures: max |GPU - OpenFst| / max(1,|s|) = {worst_fst:.3g}, max |GPU - DP64| / max(1,|s|) = {worst_dp:.3g}, "
          f"{ties} ties resolved differently from OpenFst")


def test_edge_pairs():
    """Empty sequences, a single codon, long insertions only: what the reference's composition also answers."""
    w = T.Weights("tri-mg")
    m = model_of({"model": "tri-mg", "br_len": 0.0133, "omega": 0.2, "pi": [0.308, 0.185, 0.199, 0.308], "sigma": None,
                  "gap_open": 0.001, "gap_extend": float(np.float32(1) - np.float32(1) / np.float32(6)), "bc_error": 0.0001})
    pairs = [("", ""), ("", "ACGTN"), ("ATG", ""), ("ATG", "ATG"), ("ATGGCC" * 70, "ATG"), ("ATG", "ACGT" * 100)]
    sc, ops, off, ln = m.align(*hip.triplet_encode(pairs))
    for i, (a, b) in enumerate(pairs):
        dp = T.score(a, b, w)
        assert abs(float(sc[i]) - dp) <= DP_TOL * max(1.0, dp), (i, sc[i], dp)
        x, y = T.ops_to_strings(ops[int(off[i]):int(off[i]) + int(ln[i])], a, b)
        assert abs(T.rescore(a, b, x, y, w) - dp) <= 1e-9 * max(1.0, dp), i
    m.close()


def test_batch_cli_equals_single_runs(tmp_path):
    rng = np.random.default_rng(3)
    cases = [c for c in GOLD["cases"] if c["name"].startswith("random_") and c["br_len"] == 0.0133 and c["pi"][0] == 0.308
             and c["gap_open"] == 0.001 and c["bc_error"] == 0.0001 and c["sigma"] is None and c["omega"] == 0.2]
    for model in ("tri-mg", "tri-ecm", "dna"):
        sel = [c for c in cases if c["model"] == model][:6]
        assert len(sel) >= 3
        fa = tmp_path / f"b_{model}.fasta"
        fa.write_text("".join(f">a{i}\n{c['anc']}\n>d{i}\n{c['des']}\n" for i, c in enumerate(sel)))
        r = run(fa, "-m", model, "--batch", "-o", tmp_path / f"b_{model}.json")
        assert r.returncode == 0, r.stderr
        batch = json.loads((tmp_path / f"b_{model}.json").read_text())
        assert len(batch) == len(sel)
        for i, c in enumerate(sel):
            one = tmp_path / f"one_{model}_{i}.fasta"
            one.write_text(f">a{i}\n{c['anc']}\n>d{i}\n{c['des']}\n")
            r = run(one, "-m", model, "-o", tmp_path / f"one_{model}_{i}.json")
            assert r.returncode == 0, r.stderr
            assert json.loads((tmp_path / f"one_{model}_{i}.json").read_text()) == batch[i], (model, i)
    del rng


def random_pair(rng, n_codons):
    sense = [c for c in range(64) if c not in (48, 50, 56)]
    codons = rng.choice(sense, n_codons)
    anc = "".join("ACGT"[c >> 4] + "ACGT"[(c >> 2) & 3] + "ACGT"[c & 3] for c in codons)
    des = list(anc)
    for _ in range(n_codons // 10):
        des[int(rng.integers(len(des)))] = "ACGT"[int(rng.integers(4))]
    for _ in range(max(2, n_codons // 150)):
        at = int(rng.integers(len(des) - 20))
        if rng.random() < 0.5:
            del des[at:at + int(rng.integers(1, 10))]
        else:
            des[at:at] = list("ACGT"[int(k)] for k in rng.integers(0, 4, int(rng.integers(1, 10))))
    return anc, "".join(des)


DEFAULTS = {"br_len": 0.0133, "omega": 0.2, "pi": [0.308, 0.185, 0.199, 0.308], "sigma": None, "gap_open": 0.001,
            "gap_extend": float(np.float32(1) - np.float32(1) / np.float32(6)), "bc_error": 0.0001}


@pytest.mark.parametrize("model,n_codons,full_dp", [("dna", 3334, True), ("tri-mg", 1000, True), ("tri-mg", 3334, False)])
def test_long_pair_against_float64_dp(model, n_codons, full_dp):
    """10 kb x 10 kb pairs as single pairs (53 passes of 64 codon rows, ~0.55 GB of decisions for tri-mg).  The float64
    DP costs ~400 s for a 10 kb tri-mg pair on one core, so there the check is the GPU alignment's own float64 weight
    (and the full DP runs on a 3 kb tri-mg pair and on the 10 kb dna pair)."""
    anc, des = random_pair(np.random.default_rng(11), n_codons)
    w = T.Weights(model)
    m = model_of({"model": model, **DEFAULTS})
    sc, ops, off, ln = m.align(*hip.triplet_encode([(anc, des)]))
    m.close()
    a, b = T.ops_to_strings(ops[int(off[0]):int(off[0]) + int(ln[0])], anc, des)
    re64 = T.rescore(anc, des, a, b, w)
    # fp32 summation of len_a + len_b path weights: |error| <= (len_a + len_b) * 2^-24 * score (the reference also sums in
    # fp32; measured on the 10 kb dna pair: 0.42 of 1865, 2.3e-4 relative, the same small weight rounded the same way)
    bound = (len(anc) + len(des)) * 2.0 ** -24 * max(1.0, re64)
    assert abs(float(sc[0]) - re64) <= bound, (model, sc[0], re64, bound)
    if full_dp:
        dp = T.score(anc, des, w)
        assert abs(float(sc[0]) - dp) <= bound, (model, sc[0], dp)
        assert re64 - dp <= bound, (model, re64, dp)  # optimal up to what fp32 comparisons can tell apart
