"""The host half of the device KeyFrameDatabase (eao_fusion_amd/csrc/keyframe_db_internal.h) without a device: tools/keyframe_database_walk.cpp is built with
g++ -fsanitize=address,undefined and run as a program.  It is fed the intersection arrays the yardstick (tests/keyframe_database_reference.py) computes -- what the
kernel returns on the device -- and must print the yardstick's lists, counts, float scores, candidates and used_unset, on every scene of
tests/keyframe_database_scenes.py and over seeded random sequences of add / erase / re-add / query.  The yardstick keeps a real list per word; the header keeps
none and orders by (first common word, add sequence): equality on the random sequences is the proof that the two orders are the same."""
import os
import subprocess

import numpy as np
import pytest

import keyframe_database_reference as Y
import keyframe_database_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kfdb") / "keyframe_database_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "keyframe_database_walk.cpp"), "-o", exe])
    return exe


def f32bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def f64bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def script_and_expectation(sc, results):
    """the scene's ops as the program's commands, and the lines the yardstick's results make"""
    lines, want = ["words %d" % sc["n_words"]], []
    it = iter(results)
    for op in sc["ops"]:
        if op[0] == "add":
            lines.append("add %d %d %s" % (op[1], len(op[2][0]), " ".join(str(int(w)) for w in op[2][0])))
        elif op[0] == "erase":
            lines.append("erase %d" % op[1])
        elif op[0] == "clear":
            lines.append("clear")
        else:
            _, kind, qid, bow, connected, min_score = op
            r = next(it)
            raw, res = r["raw"], r["res"]
            lines.append("query %d %d %d %d %s %d %s" % (kind, qid, f32bits(min_score), len(connected), " ".join(str(c) for c in connected), len(raw),
                                                         " ".join("%d %d %d %d" % (i, c, f, f64bits(s)) for i, c, f, s in raw)))
            want.append("sharing %d%s | %d %d %d | scored %d%s" % (
                len(res["sharing_id"]), "".join(" %d:%d" % p for p in zip(res["sharing_id"], res["sharing_words"])), res["max_common_words"], res["min_common_words"],
                res["n_scores"], len(res["scored_id"]), "".join(" %d:%d" % (i, f32bits(s)) for i, s in zip(res["scored_id"], res["scored_score"]))))
            n = len(res["scored_id"])
            nbs = [list(sc["neighbours"](i))[:Y.N_NEIGHBOURS] for i in res["scored_id"]]
            start = np.concatenate([[0], np.cumsum([len(nb) for nb in nbs])]).astype(int)
            lines.append("cand %d %d %d %d %d %s %s %s" % (kind, qid, res["min_common_words"], f32bits(min_score), n,
                                                           " ".join("%d %d" % (i, f32bits(s)) for i, s in zip(res["scored_id"], res["scored_score"])),
                                                           " ".join(str(s) for s in start), " ".join(str(i) for nb in nbs for i in nb)))
            want.append("cand %d%s | acc%s | best%s | unset %d" % (len(res["cand_id"]), "".join(" %d" % c for c in res["cand_id"]),
                                                                  "".join(" %d" % f32bits(a) for a in res["acc_score"]), "".join(" %d" % b for b in res["best_id"]),
                                                                  res["used_unset"]))
    return "\n".join(lines) + "\n", want


def run_walk(walk, script):
    out = subprocess.run([walk, "script"], input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene(walk, name):
    sc = SC.get(name)
    script, want = script_and_expectation(sc, SC.reference(name))
    got = [ln for ln in run_walk(walk, script) if not ln.startswith("compacted")]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s line %d" % (name, k)


def random_sequence(seed):
    """few word ids and few query ids: ties in the first common word, repeated query ids (0 among them), erasures, re-added ids, neighbours that are not held"""
    rs = np.random.RandomState(seed)
    n_words = int(rs.choice([12, 40, 200]))
    ops, held, gone = [], [], []
    for _ in range(90):
        u = rs.uniform()
        if u < 0.40 or not held:
            k = gone.pop(int(rs.randint(len(gone)))) if gone and rs.uniform() < 0.5 else int(rs.randint(1, 60))
            if k in held:
                continue
            ops.append(("add", k, SC.vec(rs, rs.randint(0, n_words, int(rs.randint(0, min(n_words, 25)))))))
            held.append(k)
        elif u < 0.55:
            k = held.pop(int(rs.randint(len(held))))
            gone.append(k)
            ops.append(("erase", k))
        elif u < 0.57:
            ops.append(("clear",))
            held, gone = [], []
        else:
            bow = SC.vec(rs, rs.randint(0, n_words, int(rs.randint(0, min(n_words, 25)))))
            connected = [int(c) for c in rs.randint(1, 60, int(rs.randint(0, 6)))]
            min_score = float(rs.choice([0.0, 0.05, 0.2]))
            ops.append(SC.q(int(rs.randint(2)), int(rs.randint(0, 4)), bow, connected, min_score))
    table = {k: [int(i) for i in rs.randint(1, 60, int(rs.randint(0, 13)))] for k in range(0, 61)}      # (some longer than 10: only ten are read)
    return dict(n_words=n_words, ops=ops, neighbours=lambda k: table[k])


@pytest.mark.parametrize("seed", range(12))
def test_random_sequences_prove_the_list_order(walk, seed):
    sc = random_sequence(seed)
    results = SC.run(sc, Y.Database(sc["n_words"]))
    assert len(results) > 10
    script, want = script_and_expectation(sc, results)
    got = [ln for ln in run_walk(walk, script) if not ln.startswith("compacted")]
    assert got == want


def test_the_sequences_reach_ties_repeats_and_compaction(walk):
    ties = repeats = unset = compacted = 0
    for seed in range(12):
        sc = random_sequence(seed)
        results = SC.run(sc, Y.Database(sc["n_words"]))
        compacted += sum(ln.startswith("compacted") for ln in run_walk(walk, script_and_expectation(sc, results)[0]))
        for r in results:
            firsts = [f for _, c, f, _ in r["raw"] if c > 0]
            ties += len(firsts) != len(set(firsts))
            repeats += len(r["res"]["sharing_id"]) < sum(c > 0 for _, c, _, _ in r["raw"]) and not r["op"][4]
            unset += r["res"]["used_unset"] > 0
    assert ties > 20 and repeats > 20 and unset > 5 and compacted > 3


def test_add_is_refused_as_the_header_says(walk):
    script = "words 10\nadd 1 3 1 2 3\nadd 1 2 4 5\nadd 2 2 5 4\nadd 3 2 4 4\nadd 4 1 10\nadd 5 0\nadd 6 1 9\nerase 99\nquery 1 7 0 0 3 1 0 0 0 5 0 0 0 6 0 0 0\n"
    got = run_walk(walk, script)
    assert [ln.split()[0] for ln in got] == ["refused"] * 4 + ["sharing"]      # a live id, descending ids, equal ids, a word id at n_words
    assert got[-1] == "sharing 0 | 0 0 0 | scored 0"
