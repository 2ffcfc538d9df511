// test_write_verdicts.cpp -- what the host makes of a Write schedule (no device): the verdicts of build_geometry, of
// build_read_events(any_end) and of the Rle fold, and the path the planner gives the stream, for the cases of
// tests/write_cases.py.  tests/test_write_cases.py holds each against the case's route; this is where the constants of the
// read schedule (261 / 262 / 270 / 1500 / 64 / 65274 / 32506) are pinned without a GPU.
// stdin, one case a line:  name n level strategy resume at_read p0 E0 base0 k end_1 .. end_k
//                          (resume = 1: a run that goes on at loop-top p0 with the input read to E0 and the window at base0 --
//                          GeoStart; the ends are those of the Writes behind it)
// stdout, one line a case: name geo=<0|1> body_end=<..> segs=<boundaries per segment's cluster> cl=<the boundaries, a window end
//                          as <position>w> bases=<window base behind / slide threshold at the entry of every segment>
//                          events=<0|1> nev=<..> folded=<0|1> plan_body=<..> plan_fv=<..> plan_rle=<..> lit=<bytes for the
//                          literal engine> -- the plan_* and lit fields are what plan_streams makes of the stream or the run
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../zlibstream_amd/csrc/zs_plan_key.h"
#include "../../zlibstream_amd/csrc/zs_plan.h"

using namespace zs;

int main() {
    std::string line;
    const PlanEnv env;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string name;
        int64_t n, p0, E0, base0;
        int level, strategy, resume, at_read, k;
        if (!(is >> name >> n >> level >> strategy >> resume >> at_read >> p0 >> E0 >> base0 >> k)) continue;
        std::vector<int64_t> ends((size_t)k);
        for (int i = 0; i < k; i++) is >> ends[(size_t)i];
        if (ends.empty()) ends.push_back(n);
        GeoStart gs;
        if (resume) gs.resume = true, gs.at_read = at_read != 0, gs.p0 = p0, gs.E0 = E0, gs.base0 = base0;
        const std::vector<int64_t> none;
        Geometry g;
        const bool geo = build_geometry(n, ends.size() > 1 ? ends : none, g, gs);
        std::string segs;
        for (int s = 0; geo && s < g.nsegs(); s++) segs += (s ? "," : "") + std::to_string(g.seg_cl[(size_t)s + 1] - g.seg_cl[(size_t)s]);
        std::string cl;  // the clusters' boundaries, a window end (kClWindowBit) as <position>w
        for (size_t i = 0; geo && i < g.cl.size(); i++) cl += (i ? "," : "") + std::to_string(g.cl[i] & 0x7FFFFFFFu) + ((g.cl[i] & kClWindowBit) ? "w" : "");
        std::string bases;  // per segment: window base behind its reads / slide threshold at its entry
        for (int s = 0; geo && s < g.nsegs(); s++) bases += (s ? "," : "") + std::to_string(g.seg_base[(size_t)s]) + "/" + std::to_string(g.seg_S[(size_t)s]);
        std::vector<ReadEvent> rev;
        const bool events = resume ? build_read_events(n, ends, rev, true, p0, base0) : build_read_events(n, ends, rev, true);
        // the planner's own word on these Writes
        WriteSpec ws;
        ws.ends = ends, ws.flush.assign(ends.size(), 0);
        const WriteSpec *wp[1] = {ends.size() > 1 ? &ws : nullptr};
        const void *in[1] = {(const void *)0x100000000ull};
        void *out[1] = {(void *)0x200000000ull};
        const int64_t len[1] = {n}, cap[1] = {n + n / 8 + 1024};
        FoldedWrites keep;
        PlanArgs a;
        a.n = 1, a.in = in, a.in_len = len, a.out = out, a.out_cap = cap, a.level = level, a.strategy = strategy;
        a.writes = fold_rle_writes(keep, 1, len, wp, wp[0] != nullptr, level, strategy, false, env);
        const bool folded = wp[0] && a.writes[0] && a.writes[0]->ends.size() == 1;
        Plan pl;
        std::string err;
        long body = -2, fv = -2, rle = -2, lit = -1;
        // a run that takes the stream over (GeoStart): the planner's PlanRun as the stream classes fill it in behind a flush or a
        // stop of the literal engine; a refused plan ("the run cannot go on in the bulk pipeline") leaves the fields at -2 / -1
        PlanRun ro;
        if (resume) ro.resume = true, ro.at_read = at_read != 0, ro.mid_write = !at_read, ro.p0 = p0, ro.E0 = E0, ro.base0 = base0, ro.start_block = p0, a.ro = &ro;
        if (plan_streams(pl, a, env, err)) body = pl.sd[0].body_end, fv = pl.sd[0].fv_end, rle = pl.sd[0].rle_end, lit = (long)pl.lit_bytes;
        printf("%s geo=%d body_end=%ld segs=%s cl=%s bases=%s events=%d nev=%zu folded=%d plan_body=%ld plan_fv=%ld plan_rle=%ld lit=%ld\n", name.c_str(), geo ? 1 : 0,
               geo ? (long)g.body_end : -1L, segs.empty() ? "-" : segs.c_str(), cl.empty() ? "-" : cl.c_str(), bases.empty() ? "-" : bases.c_str(), events ? 1 : 0,
               rev.size(), folded ? 1 : 0, body, fv, rle, lit);
    }
    return 0;
}
