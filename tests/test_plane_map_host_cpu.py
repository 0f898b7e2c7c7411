"""The host half of the device plane map (eao_fusion_amd/csrc/plane_map_internal.h) without a device: tools/plane_association_walk.cpp -- the reference's loops
over that header's table, with a host arena that grows and compacts as the library's does -- is built with g++ -fsanitize=address,undefined and run as a
program of its own.  It must print the yardstick's (tests/plane_association_reference.py) matches, distances, gate flags and world coefficients as bit patterns on
every scene, and the yardstick's offsets and counts over seeded random sequences of add / update / set / erase / re-add / clear at small arena sizes."""
import os
import subprocess

import numpy as np
import pytest

import plane_association_reference as Y
import plane_association_scenes as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pmap") / "plane_association_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "plane_association_walk.cpp"), "-o", exe])
    return exe


def hx(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def query_line(M, set_start, coef, cand_id, dis_th, angle_th):
    M = np.asarray(M, np.float32).reshape(-1, 16)
    ids = "-1" if cand_id is None else "%d %s" % (len(cand_id), " ".join(str(c) for c in cand_id))
    return "query %s %s %d %s %s %s %s" % (hx([dis_th]), hx([angle_th]), len(M), hx(M), " ".join(str(int(s)) for s in set_start), hx(coef), ids)


def result_line(r):
    return "match%s | mdis%s | coef%s | dis%s | gated%s" % (
        "".join(" %d" % m for m in r["match"]), "".join(" " + hx([v]) for v in r["match_dis"]), "".join(" " + hx([v]) for v in r["world_coef"].reshape(-1)),
        "".join(" " + hx([v]) for v in r["dis"].reshape(-1)), "".join(" %d" % g for g in r["gated"].reshape(-1)))


def table_line(m):
    return "table used %d dead %d live %d |%s" % (m.used, m.dead, len(m.live()), "".join(" %d:%d:%d" % (e[0], e[1], e[2]) for e in m.live()))


def run_walk(walk, script, initial=None):
    out = subprocess.run([walk, "script"] + ([str(initial)] if initial else []), input=script, capture_output=True, text=True)
    assert out.returncode == 0, "exit %d\n%s" % (out.returncode, out.stderr[-3000:])
    return out.stdout.strip().split("\n") if out.stdout.strip() else []


def quiet(lines):
    return [ln for ln in lines if not ln.startswith(("grew", "compacted"))]


@pytest.mark.parametrize("name", sorted(SC.SCENES))
def test_every_scene(walk, name):
    sc, m = SC.get(name), SC.model(SC.get(name))
    lines = ["add %d %s %d %s" % (e[0], hx(e[3]), e[2], hx(e[4])) for e in m.live()]      # the yardstick's world-frame clouds
    lines += ["table", query_line(sc["M"], sc["set_start"], sc["coef"], sc["cand_id"], sc["dis_th"], sc["angle_th"])]
    got = quiet(run_walk(walk, "\n".join(lines) + "\n", initial=64))
    assert got == [table_line(m), result_line(SC.reference(name))]


def random_sequence(seed):
    """small clouds and a small arena: growth, dead clouds, compaction, ids that come back, queries in between"""
    rs = np.random.RandomState(seed)
    m, lines, want, held, gone = Y.Model(), [], [], [], []

    def cloud():
        return SC.at_height(rs.uniform(0.0, 0.4, int(rs.randint(0, 40))), int(rs.randint(1 << 30)))

    def world():
        return np.array([0, 0, rs.choice([1.0, -1.0, 0.5]), 0], np.float32)

    for _ in range(120):
        u = rs.uniform()
        if u < 0.30 or not held:
            k = gone.pop(int(rs.randint(len(gone)))) if gone and rs.uniform() < 0.5 else int(rs.randint(1, 50))
            if k in held:
                lines.append("add %d %s 0" % (k, hx(SC.UP)))
                want.append("refused")
                continue
            w, c = world(), cloud()
            m.add(k, w, c)
            held.append(k)
            lines.append("add %d %s %d %s" % (k, hx(w), len(c), hx(c)))
        elif u < 0.50:
            k, c = held[int(rs.randint(len(held)))], cloud()
            m.update_boundary(k, c)
            lines.append("update %d %d %s" % (k, len(c), hx(c)))
        elif u < 0.55:
            k, w = held[int(rs.randint(len(held)))], world()
            m.set_world_pos(k, w)
            lines.append("setw %d %s" % (k, hx(w)))
        elif u < 0.72:
            k = held.pop(int(rs.randint(len(held)))) if rs.uniform() < 0.9 else 99
            if k != 99:
                gone.append(k)
            m.erase(k)
            lines.append("erase %d" % k)
        elif u < 0.74:
            m.clear()
            held, gone = [], []
            lines.append("clear")
        else:
            cand = None if rs.uniform() < 0.5 else [held[int(i)] for i in rs.randint(0, len(held), int(rs.randint(0, 6)))]
            coef = np.array([[0, 0, 1, -rs.uniform(0, 0.3)] for _ in range(int(rs.randint(0, 4)))], np.float32).reshape(-1, 4)
            r = Y.associate(SC.I4, None, coef, m.candidates(cand))
            lines.append(query_line(SC.I4, [0, len(coef)], coef, cand, Y.DIS_TH, Y.ANGLE_TH))
            want.append(result_line(r))
        lines.append("table")
        want.append(table_line(m))
    return "\n".join(lines) + "\n", want, m.compactions


@pytest.mark.parametrize("seed", range(8))
def test_random_sequences(walk, seed):
    script, want, _ = random_sequence(seed)
    assert quiet(run_walk(walk, script, initial=16)) == want


def doubled(start, need):
    """the smallest start * 2^k that is at least need"""
    c = start
    while c < need:
        c *= 2
    return c


def test_the_sequences_reach_growth_and_compaction(walk):
    """... and every capacity the walk prints is the storage policy's: initial * 2^k; a growth doubles the capacity it found until the points in use fit; a
    compaction leaves the smallest initial * 2^k that is at least twice the points in use of the `table` line that follows (all live by then)."""
    initial = 16
    grew = compacted = model_compactions = 0
    for seed in range(8):
        script, _, c = random_sequence(seed)
        got = run_walk(walk, script, initial=initial)
        model_compactions += c
        cap = 0      # (clear keeps the allocation)
        for i, ln in enumerate(got):
            if not ln.startswith(("grew", "compacted")):
                continue
            n = int(ln.split()[1])
            table = next(x for x in got[i + 1:] if x.startswith("table")).split()
            used, dead = int(table[2]), int(table[4])
            assert n == doubled(initial, n), (seed, i, ln)
            if ln.startswith("grew"):
                grew += 1
                assert n > cap and n >= used, (seed, i, ln, cap, used)
                if got[i + 1].startswith("table"):      # no compaction in between: `used` is what the growth had to hold
                    assert used > cap and n == doubled(cap or initial, used), (seed, i, ln, cap, used)
            else:
                compacted += 1
                assert got[i + 1].startswith("table") and dead == 0 and n == doubled(initial, 2 * used), (seed, i, ln, used, dead)
            cap = n
    assert grew > 8 and compacted > 8 and compacted == model_compactions


def test_refusals(walk):
    script = "add 1 %s 0\nadd 1 %s 0\nupdate 2 0\nsetw 2 %s\nerase 5\n%s\n" % (hx(SC.UP), hx(SC.UP), hx(SC.UP), query_line(SC.I4, [0, 1], [SC.UP], [1, 3], 0.2, 0.8))
    assert run_walk(walk, script) == ["refused"] * 4      # a live id, an update and a set of an unknown one, an unknown candidate
