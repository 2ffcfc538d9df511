"""The claims of tests/write_cases.py, held against the oracle's trace on the CPU -- every case is in the catalogue for which side
of a read rule's edge it is on, and this file is where that is checked -- then every case through the CPU model
(tests/model/zs_model.cpp: the kernels' own ZS_HD code) and through the host's verdicts (tests/cpp/test_write_verdicts.cpp:
build_geometry, build_read_events, the Rle fold and the planner itself).  The device is not involved;
tests/test_gpu_write_cases.py asks it for these bytes."""
import collections
import os
import subprocess
import zlib

import pytest

import deflate_reader as dr
import match_cases as mc
import write_cases as wc
from test_model import EXE, model  # noqa: F401  (model: the fixture that builds build/zs_model)
from write_cases import single, trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = {"event_top": 32, "lookahead": 12, "cluster": 12, "slide": 40, "tail_handover": 24, "poison": 8, "fast_events": 20, "rle_fold": 12, "resume": 22}


def test_names_counts_and_both_sides_of_every_edge():
    names = wc.case_names()
    assert len(set(names)) == len(names) == sum(COUNTS.values()) == 182
    assert dict(collections.Counter(wc.META[n][0] for n in names)) == COUNTS == wc.FAMILY_COUNTS
    sides = collections.defaultdict(set)
    for n in names:
        family, edge, side = wc.META[n]
        sides[(family, edge)].add(side)
    lost = sorted(k for k, v in sides.items() if v != {"in", "out"})
    assert not lost, lost
    assert max(len(wc.case(n)[1]) for n in names) == 133000  # every stream under 135 000 bytes
    routes = collections.Counter(wc.case(n)[7] for n in names)
    assert set(routes) == {"bulk", "bulk_tail", "literal", "poisoned", "sweeps", "folded", "resumed"}, routes
    for n in names:  # a flush mode on the first Write alone, and only in the resume family
        flushes = wc.case(n)[5]
        assert (flushes is not None) == (wc.META[n][0] == "resume") and (flushes is None or (flushes[0] in (2, 3) and not any(flushes[1:]))), n


def test_route_only_cases_are_few_and_where_they_may_be():
    """A case without a claim about its stream is allowed where the rule says who runs the stream, not what it says: the Rle fold,
    the cluster's span and count, the lengths of the tail hand-over -- and its first cluster, whose Write end cannot show in the
    stream (write_cases._tail_cases says why)."""
    assert len(wc.ROUTE_ONLY) == 22 and 4 * len(wc.ROUTE_ONLY) <= len(wc.case_names())
    for n in wc.ROUTE_ONLY:
        family, edge, _ = wc.META[n]
        assert family == "rle_fold" or (family, edge) in (("cluster", "span"), ("cluster", "count"), ("tail_handover", "length_L1"), ("tail_handover", "length_L3"),
                                                           ("tail_handover", "first_cluster")), n
        assert wc.case(n)[6] is None
    for n in ("tail_first_cluster_n723", "tail_first_cluster_n724"):  # ... the reason, held: both Writes are read at loop-top 0
        assert n in wc.ROUTE_ONLY


def test_the_first_clusters_write_end_cannot_show(oracle):
    for n in ("tail_first_cluster_n723", "tail_first_cluster_n724"):
        z, _, reads, _ = trace(oracle, n)
        assert [r[:2] for r in reads] == [(0, 200), (0, len(wc.case(n)[1]) - 200)] and z == single(oracle, n)


@pytest.mark.parametrize("family", sorted(COUNTS))
def test_claims_hold_on_the_oracles_trace_and_the_catalogue_discriminates(oracle, family):
    bad = []
    for name in wc.case_names(family):
        _, data, level, strategy, ends, flushes, claim, route = wc.case(name)
        z, t, reads, slides = trace(oracle, name)
        assert zlib.decompress(z) == data and dr.replay(dr.read(z)) == data, name
        if name in wc.ROUTE_ONLY:
            if route == "folded" and z != single(oracle, name):
                bad.append((name, "folded, but not the single Write's stream"))
            continue
        assert not any(b.kind == "stored" and b.len for b in dr.read(z)), name  # the tokens are visible (a flush marker is an empty stored block)
        if not claim(t, reads, slides):
            bad.append((name, "claim"))
        if z == single(oracle, name):
            bad.append((name, "the single Write's stream"))
        twins = wc.twins(name)
        if not twins and wc.META[name][1].split("_")[0] not in ("eq", "nil", "stale"):
            bad.append((name, "no twin"))
        for other in twins:  # what the claim names is not so on the other side of the edge
            _, t2, reads2, slides2 = trace(oracle, other)
            if claim(t2, reads2, slides2):
                bad.append((name, "the claim holds on its twin " + other))
    assert not bad, bad


def test_claims_of_the_event_top_and_slide_families_under_the_multiplicative_hash(oracle):
    assert set(wc.NOT_UNDER_HASH_VARIANT_1) <= set(wc.case_names()) and len(wc.hash_variant_names()) == 32 + 40 - len(wc.NOT_UNDER_HASH_VARIANT_1) == 64
    bad = []
    for name in wc.hash_variant_names():
        _, data, level, strategy, ends, flushes, claim, _ = wc.case(name)
        z, reads, slides = oracle.trace(data, level, strategy, wc.writes(ends), flushes, hash_variant=1)
        t = mc.tokens(dr.read(z))
        if zlib.decompress(z) != data or not (claim(t, reads, slides, 1) if wc.takes_hash_variant(name) else claim(t, reads, slides)):
            bad.append(name)
    assert not bad, bad


def test_twins_differ_by_one_write_end():
    """the sides of an edge: the same bytes, and Write lists that differ in one Write end (moved, added or dropped) or in one
    Write's size (the last Write takes up the difference)"""
    for name in wc.case_names():
        ea = wc.case(name)[4]
        for other in wc.twins(name):
            eb = wc.case(other)[4]
            a, b = wc.writes(ea), wc.writes(eb)
            one_end = len(set(ea) ^ set(eb)) in (1, 2) and abs(len(ea) - len(eb)) <= 1 and len(set(ea) - set(eb)) <= 1 and len(set(eb) - set(ea)) <= 1
            one_size = len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 2 and a[-1] != b[-1]
            assert ea != eb and (one_end or one_size), (name, other)


# ------------------------------------------------------------------ the CPU model
def _model(path, level, strategy, mode, wspec, flush=0, env=None):
    cmd = [EXE, path, str(level), str(strategy), mode, wspec, str(flush)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env) if env else None)
    assert r.returncode == 0 and "PASS" in r.stdout, (cmd, r.stdout[-500:])
    return r.stdout


@pytest.mark.parametrize("family", sorted(COUNTS))
def test_cases_through_the_cpu_model(model, tmp_path, family):
    """Levels 4-9 in the chunked form; levels 1-3 through the sweeps and the rounds over chunks of 1024 and 2048 positions; the
    literal routes through the incremental literal engine as well; Rle through the runs' form (a Write list sends the model to
    the literal engine: the fold is the planner's); the resume family in the model's `resume` mode: the flushed Write on the
    literal engine, the run behind it laid out by build_geometry with GeoStart::at_read on that engine's chains.  The model
    compares symbols, blocks, event loop-tops and bytes with the oracle itself; `tail_from=0` -- nothing parsed in the parallel
    form -- appears exactly for the literal routes, and `not a schedule for the bulk path` exactly for those of the resume family at
    levels 4-9."""
    from concurrent.futures import ThreadPoolExecutor
    jobs = []
    with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:
        for name in wc.case_names(family):
            _, data, level, strategy, ends, flushes, _, route = wc.case(name)
            path = tmp_path / name
            path.write_bytes(data)
            wspec = ",".join(map(str, wc.writes(ends)))
            if flushes:
                jobs.append((name, route, "resume", level, pool.submit(_model, str(path), level, strategy, "resume", wspec, flushes[0])))
                continue
            if strategy == mc.RLE:
                modes = [("rle", None)]
            elif level >= 4:
                modes = [("chunk", None)]
            else:
                modes = [("fsweep", None), ("frounds", {"ZS_FR_CHUNK": "1024"}), ("frounds", {"ZS_FR_CHUNK": "2048"})]
            if route == "literal":
                modes.append(("inc", None))
            for mode, env in modes:
                jobs.append((name, route, mode, level, pool.submit(_model, str(path), level, strategy, mode, wspec, 0, env)))
        bad = []
        for name, route, mode, level, f in jobs:
            out = f.result()
            if mode == "resume":
                if level >= 4 and (("not a schedule for the bulk path" in out) != (route == "literal") or "forward pointer" in out):
                    bad.append((name, mode, out[-200:]))
                continue
            if mode in ("inc", "rle") or route == "poisoned":
                if route == "poisoned" and "poisoned" not in out:
                    bad.append((name, mode, "not flagged"))
                continue
            if ("tail_from=0\n" in out) != (route == "literal") or "poisoned" in out:
                bad.append((name, mode, out[-200:]))
    assert not bad, bad


def test_a_run_behind_a_stop_of_the_literal_engine_in_the_model(model, tmp_path):
    """The other way a run goes on (GeoStart without at_read): the model's `resume` mode without a flush stops the literal engine at
    the first clean loop-top behind F and hands the rest to the chunked form.  Where the engine stops is its own affair, so no
    Write list puts E0 - p0 on 261 / 262: that edge is the verdict program's (test_geostart_verdicts)."""
    for name, F in (("gap_270_L6", 30000), ("slide_end_65535_L6", 50000)):
        path = tmp_path / name
        path.write_bytes(wc.case(name)[1])
        out = _model(str(path), 6, 0, "resume", str(F))
        assert "mode=resume stop at" in out and "tail_from=0" not in out, out


# ------------------------------------------------------------------ the host's verdicts
def _verdict_exe():
    exe = os.path.join(ROOT, "build", "test_write_verdicts")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_write_verdicts.cpp")], check=True)
    return exe


def _verdicts_of(exe, rows):
    r = subprocess.run([exe], input="\n".join(rows) + "\n", capture_output=True, text=True, check=True)
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        out[f[0]] = dict(kv.split("=", 1) for kv in f[1:])
    return out


@pytest.fixture(scope="module")
def verdicts(oracle):
    rows = []
    for name in wc.case_names():
        _, data, level, strategy, ends, flushes, _, _ = wc.case(name)
        if flushes:  # the run behind the flushed first Write: loop-top and data end at the flush, the window where the oracle has it
            F = ends[0]
            base0 = wc.reads_at(trace(oracle, name)[2], F)[0][3]
            rows.append("%s %d %d %d 1 1 %d %d %d %d %s" % (name, len(data), level, strategy, F, F, base0, len(ends) - 1, " ".join(map(str, ends[1:]))))
        else:
            rows.append("%s %d %d %d 0 0 0 0 0 %d %s" % (name, len(data), level, strategy, len(ends), " ".join(map(str, ends))))
    out = _verdicts_of(_verdict_exe(), rows)
    assert set(out) == set(wc.case_names())
    return out


def test_host_verdicts_against_the_routes(verdicts):
    """build_geometry (accepted, body_end, boundaries per segment), build_read_events(any_end), the Rle fold and what the
    planner makes of them, against the case's route: the constants 261 / 262 / 270 / 1500 / 64 / 65274 / 32506 without a GPU."""
    bad = []
    for name in wc.case_names():
        _, data, level, strategy, ends, flushes, _, route = wc.case(name)
        v, n = verdicts[name], len(data)
        geo, body, events, folded = v["geo"] == "1", int(v["body_end"]), v["events"] == "1", v["folded"] == "1"
        plan_body, plan_fv, plan_rle, lit = int(v["plan_body"]), int(v["plan_fv"]), int(v["plan_rle"]), int(v["lit"])
        if flushes:  # the planner takes the run (levels 4-9: build_geometry with GeoStart; levels 1-3: the sweeps from the flush) or refuses it
            want = (n - 262, -1) if level >= 4 else (-1, n - 262)
            ok = route in ("resumed", "literal") and (plan_body, plan_fv) == (want if route == "resumed" else (-2, -2)) and (level <= 3 or geo == (route == "resumed"))
        elif strategy == mc.RLE:
            ok = (folded, plan_rle >= 0, lit) == ((True, True, 0) if route == "folded" else (False, False, n - 261))
        elif level >= 4:
            if route in ("bulk", "poisoned"):
                ok = geo and body == n - 262 == plan_body and lit == 0
            elif route == "bulk_tail":
                ok = geo and 262 <= body < n - 262 and body == plan_body and lit == 0
            else:
                ok = route == "literal" and not geo and plan_body == -1 and lit == n - 261
            if geo:
                want = wc.expected_segments(n, ends)
                got = [int(x) for x in v["segs"].split(",")]
                ok = ok and (got == want if route != "bulk_tail" else got == want[:len(got)] and len(got) == len(want) - 1)
        else:
            ok = route in ("sweeps", "literal") and (plan_fv, lit) == ((n - 262, 0) if route == "sweeps" else (-1, n - 261))
            ok = ok and (len(ends) == 1 or events == (route == "sweeps"))
        if not ok:
            bad.append((name, route, v))
    assert not bad, bad


def test_host_verdicts_name_windows_and_bases(verdicts):
    """A Write that ends on a window end is a Write end (kClWindowBit clear: no `w`); one that ends a byte behind it leaves the
    window end in the list; behind a second window's events the base is 65536 and the slide threshold at their entry 32768 + 65274."""
    assert "65536," in verdicts["slide_end_65536_L6"]["cl"] + "," and "65536w" not in verdicts["slide_end_65536_L6"]["cl"]
    assert "65536w,65537" in verdicts["slide_end_65537_L6"]["cl"]
    assert "65274,65536w" in verdicts["slide_end_65274_L6"]["cl"] and "65273,65536w" in verdicts["slide_end_65273_L6"]["cl"]
    assert "98042,98304w" in verdicts["slide_end_98042_L6"]["cl"]
    assert "65536/98042" in verdicts["slide_end_98042_L6"]["bases"].split(",")
    assert "32768/65274" in verdicts["slide_end_65274_L6"]["bases"].split(",")
    # a run flushed at 65274 starts in the window the flush slid: base 32768, its first segment slides at 32768 + 65274
    assert verdicts["resume_flush_at_65274_L6"]["bases"].split(",")[0] == "32768/98042" and verdicts["resume_flush_at_65273_L6"]["bases"].split(",")[0] == "32768/65274"


def test_geostart_verdicts():
    """GeoStart's own edges, which no stream reaches through the stream classes (the flush's last pass through the loop slides a
    window that stands on the threshold; the literal engine stops where it has a full lookahead): a run at a read with p0 = 65273 /
    65274 in a window at base 0, a run in the middle of a Write with E0 - p0 = 262 / 261, and a run of 524 / 523 bytes."""
    rows = ["p0_65273 200000 6 0 1 1 65273 65273 0 1 200000", "p0_65274 200000 6 0 1 1 65274 65274 0 1 200000",
            "mid_262 200000 6 0 1 0 70000 70262 32768 1 200000", "mid_261 200000 6 0 1 0 70000 70261 32768 1 200000",
            "run_524_L6 67000 6 0 1 1 66476 66476 32768 1 67000", "run_523_L6 67000 6 0 1 1 66477 66477 32768 1 67000",
            "run_524_L1 67000 1 0 1 1 66476 66476 32768 1 67000", "run_523_L1 67000 1 0 1 1 66477 66477 32768 1 67000"]
    v = _verdicts_of(_verdict_exe(), rows)
    for a, b in (("p0_65273", "p0_65274"), ("mid_262", "mid_261"), ("run_524_L6", "run_523_L6")):
        assert (v[a]["geo"], v[a]["plan_body"], v[b]["geo"], v[b]["plan_body"]) == ("1", str(int(rows[0].split()[1]) - 262 if a[0] != "r" else 67000 - 262), "0", "-2"), (a, b)
    assert (v["run_524_L1"]["plan_fv"], v["run_523_L1"]["plan_fv"]) == ("66738", "-2")
    assert v["mid_262"]["segs"].split(",")[0] == "0"  # the stretch without events in front of the first cluster
