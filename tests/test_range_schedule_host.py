"""The range-correction schedules of the forward 64-bit kernels, proved on the CPU: tests/cpp/range_schedule_probe.hip
prints kern::PassSched as compiled from the headers for every pass shape lazy_launch_impl.hpp instantiates (16 q, 31 q,
8 q and 4 q ranges) and what the host's run-time twin reports for the plans of the rings 2^13 .. 2^18; this file replays
every table with exact integer bounds per register.  Random data never reaches these ranges -- this is the test that
holds them.  Weights of a correction, in VALU instructions per value: conditional subtraction 4, quotient estimate 5."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
EPT = 16
COST_CSUB, COST_EST, EST = 4, 5, -1
EST_DOMAIN = 32  # Mod64::reduce_2q: x < 32 q (pinned word for word by tests/test_gpu_lazy_arith.py)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    lib = os.path.join(ROOT, "gpu-ntt_amd", "lib")
    if not os.path.exists(os.path.join(lib, "libgpuntt.so")):
        from conftest import load_pkg
        load_pkg().build_library()
    exe = str(tmp_path_factory.mktemp("range_probe") / "range_schedule_probe")
    subprocess.check_call([HIPCC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "range_schedule_probe.hip"), "-O1",
                           "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gpu-ntt_amd", "csrc"), "-L" + lib, "-lgpuntt", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib", "-Wno-unused-result", "-o", exe], timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    scheds, twins, caps, plans = [], {}, {}, []
    for ln in r.stdout.splitlines():
        f = ln.split()
        if f[0] == "S":
            keys = ("lim", "tile", "tlog", "contig", "k", "inb", "cap", "last", "est", "limit", "tb", "final", "nr")
            s = {k: (v if k == "tile" else int(v)) for k, v in zip(keys, f[1:])}
            s["rounds"] = []
            scheds.append(s)
        elif f[0] == "R":
            parts = ln[2:].split("|")
            stages, bin_ = (int(v) for v in parts[0].split())
            st = [[int(v) for v in p.split()] for p in parts[1:1 + stages]]
            bout = [int(v) for v in parts[1 + stages].split()]
            assert all(len(s) == 1 + EPT // 2 for s in st) and len(bout) == EPT
            scheds[-1]["rounds"].append({"bin": bin_, "stages": [(s[0], s[1:]) for s in st], "bout": bout})
        elif f[0] == "T":
            twins[tuple(int(v) for v in f[1:7])] = int(f[7])
        elif f[0] == "C":
            caps[int(f[1])] = int(f[2])
        elif f[0] == "P":
            plans.append({"lim": int(f[1]), "n": int(f[2]), "polys": int(f[3]), "tl": int(f[4]), "passes": []})
            assert int(f[5]) >= 1
        elif f[0] == "Q":
            keys = ("contig", "k", "tlp", "first", "last", "in_b", "inst", "cap", "out")
            plans[-1]["passes"].append(dict(zip(keys, (int(v) for v in f[1:]))))
    assert all(len(s["rounds"]) == s["nr"] for s in scheds)
    return scheds, twins, caps, plans


def key_of(s):
    return (s["lim"], s["tlog"], s["contig"], s["k"], s["inb"], s["cap"])


def replay(s):
    """exact bounds per register through the schedule; returns (hand-off bound, cost per U value, correction stages)"""
    limit, tb = s["limit"], s["tb"]
    b = [s["inb"]] * EPT
    cost = nstage = 0
    assert sum(len(r["stages"]) for r in s["rounds"]) == s["k"]
    for r in s["rounds"]:
        assert r["bin"] >= max(b)
        for jb, kus in r["stages"]:
            assert 0 <= jb < 4
            touched = set()
            for h, ku in enumerate(kus):
                j0 = (h & ((1 << jb) - 1)) | ((h >> jb) << (jb + 1))
                j1 = j0 | (1 << jb)
                touched |= {j0, j1}
                u = b[j0]
                if ku == EST:
                    assert s["est"] and u <= EST_DOMAIN and tb == 4, (key_of(s), "estimate outside its domain")
                    u = min(u, 2)
                elif ku > 0:
                    assert u <= 2 * ku, (key_of(s), "csub<%d> on a value below %d q" % (ku, u))
                    u = min(u, ku)
                else:
                    assert ku == 0
                assert u + tb <= limit, (key_of(s), "U + T passes the range")
                b[j0] = b[j1] = u + tb
            assert len(touched) == EPT
            if s["est"]:  # whole-pass plans: one correction for the whole stage
                assert len(set(kus)) == 1
            cost += max({0: 0, EST: COST_EST}.get(ku, COST_CSUB) for ku in kus)
            nstage += any(ku != 0 for ku in kus)
        assert all(st >= ex for st, ex in zip(r["bout"], b)), (key_of(s), "a stated bound below the exact one")
        b = list(r["bout"])  # what the next round (and the normalisation) is compiled for
    return max(b), cost, nstage


def old_cost(inb, k, limit, tb):
    """ct_plan at every stage (lazy.hpp: csub_k halves the bound to a power of two): the schedule before whole-pass plans"""
    cost, b = 0, inb
    for _ in range(k):
        if b + tb > limit:
            p = 1
            while p < b:
                p <<= 1
            b = p // 2
            cost += COST_CSUB
        b += tb
    return b, cost


def test_every_schedule_keeps_its_ranges(probe):
    scheds, twins, caps, _ = probe
    assert {s["lim"] for s in scheds} == {0, 31, 8, 4} and len(scheds) > 100
    assert {s["tile"] for s in scheds if s["k"] == 10 and s["contig"] and s["inb"] > 1 and s["tlog"] == 12} == {"p1", "p4"}
    for s in scheds:
        out, cost, _ = replay(s)
        assert s["final"] >= out and s["final"] <= s["limit"]
        assert s["final"] <= (s["cap"] or s["limit"]), (key_of(s), "hand-off above the cap")
        if s["last"]:  # normalize<B>: 64-bit words take the estimate for B > 4
            assert s["final"] <= (EST_DOMAIN if s["tb"] == 4 else 4)
        assert s["est"] == (s["lim"] in (0, 31))
        if s["est"]:
            assert twins[key_of(s)] == s["final"], (key_of(s), "the run-time twin reports another hand-off")
        ofinal, ocost = old_cost(s["inb"], s["k"], s["limit"], s["tb"])
        if not s["est"]:
            assert (cost, s["final"]) == (ocost, ofinal), (key_of(s), "a family without whole-pass plans changed")
        elif s["cap"] == 0:
            assert cost <= ocost, (key_of(s), cost, ocost)
    assert caps == {31: 19, 0: 12}


def test_the_caps_follow_the_rule(probe):
    """cap = the largest input bound from which the 10-stage last pass needs its fewest correction stages"""
    scheds, _, caps, _ = probe
    by = {key_of(s): s for s in scheds if s["tile"] == "p1"}
    for lim, limit in ((31, 31), (0, 16)):
        at_cap = replay(by[(lim, 12, 1, 10, caps[lim], 0)])
        at_lim = replay(by[(lim, 12, 1, 10, limit, 0)])
        assert at_cap[2] < at_lim[2] and at_cap[1] < at_lim[1]
    assert replay(by[(31, 12, 1, 10, 19, 0)])[2] == 1  # 19, 23, 27, 31 -> estimate -> 6 .. 30


def test_the_host_reports_what_the_kernels_hand_over(probe):
    scheds, _, caps, plans = probe
    by = {key_of(s): s for s in scheds if s["tile"] == "p1"}
    assert {p["n"] for p in plans} == set(range(13, 19)) and {p["lim"] for p in plans} == {0, 31}
    seen_c2 = False
    for pl in plans:
        limit = 31 if pl["lim"] == 31 else 16
        bound, new_cost, was_cost, was_bound = 1, 0, 0, 1
        for i, q in enumerate(pl["passes"]):
            assert q["first"] == (i == 0) and q["last"] == (i == len(pl["passes"]) - 1)
            assert q["in_b"] == bound and q["in_b"] <= q["inst"], (pl, "a kernel compiled for less than it receives")
            s = by[(pl["lim"], q["tlp"], q["contig"], q["k"], q["inst"], q["cap"])]  # KeyError: a shape nobody instantiates
            assert s["last"] == q["last"] and s["final"] == q["out"], (pl, q, s["final"])
            out, cost, nstage = replay(s)
            assert out <= q["out"]
            bound = q["out"]
            new_cost += cost
            # the schedule this plan ran before: ct_plan per stage; the 31 q range tracked the bound and had the 10-stage
            # last pass for 27 q, everything else was compiled for 1 (first pass) or the range limit
            was_in = 1 if i == 0 else limit
            if pl["lim"] == 31 and q["contig"] and q["k"] == 10 and q["tlp"] == 12 and i > 0 and was_bound <= 27:
                was_in = 27
            was_cost += old_cost(was_in, q["k"], limit, 4)[1]
            was_bound = old_cost(was_in, q["k"], limit, 4)[0]
            if pl["lim"] == 31 and pl["n"] == 16 and q["last"] and len(pl["passes"]) == 2:
                seen_c2 = True  # the flagship plan: 6 strided + 10 contiguous stages
                assert (pl["passes"][0]["k"], q["k"], q["inst"]) == (6, 10, caps[31]) and nstage == 1
                assert pl["passes"][0]["cap"] == caps[31]
        assert new_cost <= was_cost, (pl, new_cost, was_cost)
    assert seen_c2
