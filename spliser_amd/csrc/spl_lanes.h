// spl_lanes.h -- which stream a counting pass runs on and which recorded events it must wait for, as plain C++ with no HIP
// types: spl_capi.cpp turns the answer into hipStreamWaitEvent / hipEventRecord calls, the host compiles the same text
// (spl_lanes_plan_host, tests/hostsim/lanes_rule_asan.cpp) and the CPU suite holds it to a hazard checker (tests/lanecases.py).
//
// Streams: lane 0 (the context's main stream), lane 1 (a second stream for the slots kernel, the range kernel and the tail of a
// read set: the shards of a sample share nothing and run side by side), and the tail stream (literal kernel, scan + SSE of the
// passes on lane 0, in launch order, beside the next range kernel).  A pass over (table, set) on lane L conflicts with
//   - the last range kernel on the table (passes over one table stay in launch order whatever their lanes),
//   - the tail two passes back on the table: it cleared the counter copy this pass takes (three copies a table),
//   - the tail two passes back on the set: it read the queue buffer this pass writes (two buffers a set),
// its tail with the last tail on the table and on the set (they share the scan's outputs, and a tail clears the copy the tail
// before it on the table has read), and a set's slots kernel with the last tail on the set (its literal kernel reads the chunk
// descriptors the slots kernel writes; that tail stands behind its range kernel, which read the slots).  Every object remembers those events; an event carries a
// CLOCK -- per stream, how many of its launches are over once the event has fired -- and so does every stream: how much of each
// stream its next launch stands behind.  A wait is queued only for an event whose clock the stream's own does not cover yet.
//
// Everything else the library queues goes on the main stream behind a JOIN (the main stream waits for the newest tail of the tail
// stream and of lane 1 and, where lane 1 has work no tail stands behind, for a marker recorded on lane 1).  Lane 1's first launch after a barrier, or after such
// other work, is SETTLED behind the main stream as it stood then: through the newest tail of that moment where that covers it
// (the benchmark's step: no marker packet in the main queue), through a marker on the main stream otherwise.
#ifndef SPL_LANES_H
#define SPL_LANES_H
#include <stdint.h>

enum { SPL_LANE_MAIN = 0, SPL_LANE_SIDE = 1, SPL_LANE_TAIL = 2, SPL_LANE_STREAMS = 3 };
enum { SPL_LEV_NONE = 0, SPL_LEV_RANGE = 1, SPL_LEV_TAIL = 2, SPL_LEV_MAIN = 3, SPL_LEV_SIDE = 4, SPL_LEV_STAIL = 5 }; // kinds of recorded events (TAIL: a tail on the tail stream, STAIL: on lane 1)
enum { SPL_LOP_WAIT = 1, SPL_LOP_RECORD = 2 };
enum { SPL_LANE_RING = 8 };      // passes whose range and tail events the context keeps (older ones: the newest tail stands for them)
enum { SPL_LANE_MAX_OPS = 12 };

struct spl_lane_clock { uint64_t t[SPL_LANE_STREAMS]; };
struct spl_lane_event { int32_t kind, via; uint64_t seq; spl_lane_clock at; }; // RANGE: seq = the pass, via = the kind of its tail's event; TAIL / STAIL / MAIN / SIDE: the number among its kind
struct spl_lane_table { spl_lane_event range, tail_prev, tail_last; };
struct spl_lane_set { spl_lane_event tail_prev, tail_last; int32_t lane, slots_pending; };
struct spl_lane_op { int32_t op, stream, kind; uint64_t seq; };
struct spl_lane_plan { int32_t lane, piped, n_ops, n_after, n_mid, tail_stream; uint64_t pass, tail_seq; // (the last n_after ops: behind the call's own launches; the n_mid before them: between the range kernel and the tail)
    spl_lane_op ops[SPL_LANE_MAX_OPS]; };
struct spl_lanes {
    int32_t two, tail, foreign_main; // a second lane; a tail stream; the main stream is the caller's (work on it that this does not see)
    spl_lane_clock now[SPL_LANE_STREAMS], side_floor;
    spl_lane_event tail_new, stail_new, main_ev, side_ev, floor_tail; // (tail_new / stail_new: the newest tail on the tail stream / on lane 1)
    uint64_t n_pass, n_tail, n_stail, n_main, n_side;
    int32_t range_lane;              // the most recently launched range kernel: its lane and its set
    const spl_lane_set *range_set;
};

static inline void spl_lanes_init(spl_lanes *L, int two, int tail, int foreign_main)
{
    *L = spl_lanes();
    L->tail = tail ? 1 : 0;
    L->two = (two && tail) ? 1 : 0;
    L->foreign_main = foreign_main ? 1 : 0;
}
static inline void spl_lane_table_init(spl_lane_table *t) { *t = spl_lane_table(); }
static inline void spl_lane_set_init(spl_lane_set *s) { *s = spl_lane_set(); }

static inline bool spl_lane_covered(const spl_lane_clock &a, const spl_lane_clock &by)
{
    for (int k = 0; k < SPL_LANE_STREAMS; ++k) if (a.t[k] > by.t[k]) return false;
    return true;
}
static inline void spl_lane_absorb(spl_lane_clock &into, const spl_lane_clock &a)
{
    for (int k = 0; k < SPL_LANE_STREAMS; ++k) if (a.t[k] > into.t[k]) into.t[k] = a.t[k];
}
static inline void spl_lane_emit(spl_lane_plan *p, int op, int stream, const spl_lane_event &ev)
{
    if (p->n_ops < SPL_LANE_MAX_OPS) { spl_lane_op &o = p->ops[p->n_ops]; o.op = op; o.stream = stream; o.kind = ev.kind; o.seq = ev.seq; }
    p->n_ops++; // (more than SPL_LANE_MAX_OPS cannot come of one call: the caller asserts it)
}
// `stream` waits for `ev` unless it stands behind it already.  An event whose slot of its ring has been taken again is stood for
// by the newest tail of the stream its pass's tail ran on (a stream's tails run in order, each behind its range kernel); an earlier
// marker by the stream's latest one.
static inline void spl_lane_wait(spl_lanes *L, spl_lane_plan *p, int stream, spl_lane_event ev)
{
    if (ev.kind == SPL_LEV_NONE || spl_lane_covered(ev.at, L->now[stream])) return;
    if (ev.kind == SPL_LEV_RANGE && ev.seq + SPL_LANE_RING <= L->n_pass) ev = ev.via == SPL_LEV_STAIL ? L->stail_new : L->tail_new;
    if (ev.kind == SPL_LEV_TAIL && ev.seq + SPL_LANE_RING <= L->n_tail) ev = L->tail_new;
    if (ev.kind == SPL_LEV_STAIL && ev.seq + SPL_LANE_RING <= L->n_stail) ev = L->stail_new;
    if (ev.kind == SPL_LEV_MAIN) ev = L->main_ev;
    if (ev.kind == SPL_LEV_SIDE) ev = L->side_ev;
    spl_lane_emit(p, SPL_LOP_WAIT, stream, ev);
    spl_lane_absorb(L->now[stream], ev.at);
}
static inline void spl_lane_record_main(spl_lanes *L, spl_lane_plan *p)
{
    L->main_ev.kind = SPL_LEV_MAIN; L->main_ev.at = L->now[SPL_LANE_MAIN];
    if (!L->two) return; // (one lane: whoever might ask stands behind the main stream already, nothing to record)
    L->main_ev.seq = ++L->n_main;
    spl_lane_emit(p, SPL_LOP_RECORD, SPL_LANE_MAIN, L->main_ev);
}
// The main stream behind everything launched so far.
static inline void spl_lane_join(spl_lanes *L, spl_lane_plan *p)
{
    if (!L->tail) return;
    spl_lane_wait(L, p, SPL_LANE_MAIN, L->tail_new);
    if (L->now[SPL_LANE_SIDE].t[SPL_LANE_SIDE] > L->now[SPL_LANE_MAIN].t[SPL_LANE_SIDE]) spl_lane_wait(L, p, SPL_LANE_MAIN, L->stail_new);
    if (L->now[SPL_LANE_SIDE].t[SPL_LANE_SIDE] > L->now[SPL_LANE_MAIN].t[SPL_LANE_SIDE]) { // (a slots kernel no pass followed)
        L->side_ev.kind = SPL_LEV_SIDE; L->side_ev.seq = ++L->n_side; L->side_ev.at = L->now[SPL_LANE_SIDE];
        spl_lane_emit(p, SPL_LOP_RECORD, SPL_LANE_SIDE, L->side_ev);
        spl_lane_wait(L, p, SPL_LANE_MAIN, L->side_ev);
    }
}
// Lane 1's next launch stands behind the main stream as it was at the last barrier / the last other work on it.
static inline void spl_lane_settle(spl_lanes *L, spl_lane_plan *p, int lane)
{
    if (lane != SPL_LANE_SIDE || spl_lane_covered(L->side_floor, L->now[SPL_LANE_SIDE])) return;
    spl_lane_wait(L, p, SPL_LANE_SIDE, L->floor_tail);
    if (!spl_lane_covered(L->side_floor, L->now[SPL_LANE_SIDE])) {
        spl_lane_clock with = L->now[SPL_LANE_SIDE];
        spl_lane_absorb(with, L->main_ev.at);
        if (L->main_ev.kind == SPL_LEV_NONE || !spl_lane_covered(L->side_floor, with)) spl_lane_record_main(L, p); // (late: orders more than it must)
        spl_lane_wait(L, p, SPL_LANE_SIDE, L->main_ev);
    }
}
static inline void spl_lane_floor(spl_lanes *L)
{
    L->side_floor = L->now[SPL_LANE_MAIN];
    L->floor_tail = L->tail_new;
}

// spl_pass_barrier (and nothing queued): whatever is launched afterwards, on either lane, starts after everything before it.
static inline void spl_lanes_barrier(spl_lanes *L, spl_lane_plan *p)
{
    *p = spl_lane_plan();
    if (!L->tail) return;
    spl_lane_join(L, p);
    if (!L->two) return;
    if (L->foreign_main) L->now[SPL_LANE_MAIN].t[SPL_LANE_MAIN]++; // (what the caller queued on its stream)
    spl_lane_floor(L);
    spl_lane_clock with = L->now[SPL_LANE_SIDE]; // (what lane 1 will stand behind with the events there are: the newest tail, the last marker)
    spl_lane_absorb(with, L->tail_new.at);
    spl_lane_absorb(with, L->main_ev.at);
    if (!spl_lane_covered(L->side_floor, with)) spl_lane_record_main(L, p);
}
// A join alone (spl_sync, the timers, the downloads before they queue their copies).
static inline void spl_lanes_join(spl_lanes *L, spl_lane_plan *p) { *p = spl_lane_plan(); spl_lane_join(L, p); }
// Any other work the library queues on the main stream: behind a join, and lane 1's next launch behind it.
// (joined = 0: work on an object nothing launched so far touches -- spl_reads_finish's first layout -- which needs no join.)
static inline void spl_lanes_main_work(spl_lanes *L, int joined, spl_lane_plan *p)
{
    *p = spl_lane_plan();
    if (!L->tail) return;
    if (joined) spl_lane_join(L, p);
    L->now[SPL_LANE_MAIN].t[SPL_LANE_MAIN]++;
    spl_lane_floor(L);
}
// The host has waited for the main stream behind a join: everything launched so far is over, whichever stream asks.
static inline void spl_lanes_host_synced(spl_lanes *L)
{
    spl_lane_clock all = L->now[0];
    for (int s = 1; s < SPL_LANE_STREAMS; ++s) spl_lane_absorb(all, L->now[s]);
    for (int s = 0; s < SPL_LANE_STREAMS; ++s) L->now[s] = all;
}

// spl_reads_relayout: the set's lane -- the one the most recently launched range kernel is NOT on; its own again if that pass was
// over this very set (or a slots kernel of the set is still waiting for its pass) -- and what the slots kernel waits for there.
// A set that is not fused is laid out on the main stream.
static inline void spl_lanes_relayout(spl_lanes *L, spl_lane_set *set, int fused, spl_lane_plan *p)
{
    *p = spl_lane_plan();
    int lane = SPL_LANE_MAIN;
    if (L->two && fused) {
        if (set->slots_pending || L->range_set == set) lane = set->lane;
        else if (L->range_set) lane = 1 - L->range_lane;
    }
    p->lane = lane;
    if (!L->tail) return;
    spl_lane_settle(L, p, lane);
    spl_lane_wait(L, p, lane, set->tail_last);
    L->now[lane].t[lane]++;
    set->lane = lane;
    set->slots_pending = 1;
}

// spl_count_launch.  piped_wanted: the range kernel on a counter copy that is clean (the caller's bookkeeping).  Piped: the
// range kernel on the set's lane, the tail on the tail stream behind the range kernel's event.  Otherwise (pair kernel, first
// pass after one, no tail stream): everything in order on the main stream behind a join, and a marker behind it.
static inline void spl_lanes_count(spl_lanes *L, spl_lane_table *table, spl_lane_set *set, int piped_wanted, spl_lane_plan *p)
{
    *p = spl_lane_plan();
    if (!L->tail) return;
    if (!piped_wanted) {
        spl_lane_join(L, p);
        L->now[SPL_LANE_MAIN].t[SPL_LANE_MAIN]++;
        const int32_t n_before = p->n_ops;
        spl_lane_record_main(L, p);
        p->n_after = p->n_ops - n_before;
        spl_lane_floor(L);
        table->range = table->tail_prev = table->tail_last = L->main_ev;
        set->tail_prev = set->tail_last = L->main_ev;
        set->lane = SPL_LANE_MAIN; set->slots_pending = 0;
        L->range_lane = SPL_LANE_MAIN; L->range_set = set;
        return;
    }
    const int lane = L->two ? set->lane : SPL_LANE_MAIN;
    p->lane = lane; p->piped = 1; p->pass = L->n_pass;
    spl_lane_settle(L, p, lane);
    spl_lane_wait(L, p, lane, table->range);
    spl_lane_wait(L, p, lane, table->tail_prev);
    spl_lane_wait(L, p, lane, set->tail_prev);
    L->now[lane].t[lane]++;
    // The tail of a pass on lane 1 stays on lane 1, behind its range kernel in stream order: on the one tail stream it would stand
    // behind the tail of the pass launched before it, which waits for a range kernel that may well end later (the benchmark's
    // large shard, launched first).  Tails on ONE table or set stay in launch order: they share the scan's outputs, and a tail
    // clears the counter copy the tail before it on the table has just read.
    const int ts = lane == SPL_LANE_SIDE ? SPL_LANE_SIDE : SPL_LANE_TAIL;
    spl_lane_event r; r.kind = SPL_LEV_RANGE; r.via = ts == SPL_LANE_SIDE ? SPL_LEV_STAIL : SPL_LEV_TAIL; r.seq = L->n_pass; r.at = L->now[lane];
    if (ts == SPL_LANE_TAIL) spl_lane_absorb(L->now[SPL_LANE_TAIL], r.at); // (the tail stream waits for the range kernel's own stop event)
    const int32_t n_head = p->n_ops;
    spl_lane_wait(L, p, ts, table->tail_last);
    spl_lane_wait(L, p, ts, set->tail_last);
    p->n_mid = p->n_ops - n_head;
    p->tail_stream = ts;
    L->now[ts].t[ts]++;
    spl_lane_event t; t.kind = r.via; t.via = 0; t.seq = ts == SPL_LANE_SIDE ? L->n_stail++ : L->n_tail++; t.at = L->now[ts];
    p->tail_seq = t.seq;
    table->range = r; table->tail_prev = table->tail_last; table->tail_last = t;
    set->tail_prev = set->tail_last; set->tail_last = t;
    set->slots_pending = 0;
    if (ts == SPL_LANE_SIDE) L->stail_new = t; else L->tail_new = t;
    L->range_lane = lane; L->range_set = set;
    L->n_pass++;
}

// The rule over a sequence of calls (spl_lanes_plan_host): calls[4 * i] = kind, a, b, c --
//   0 relayout(set a, fused b)   1 count(table a, set b, piped_wanted c)   2 barrier   3 download(table a): join, copies, the host waits
//   4 other work on the main stream (a: behind a join)
// out[i * stride]: lane, piped, n_ops, n_after, n_mid, the tail's stream, then n_ops times (op, stream, kind, seq); stride = 6 + 4 * SPL_LANE_MAX_OPS.  Returns 0, or
// -1 for a call it does not know or an object out of range.
static inline int spl_lanes_plan(int two, int tail, int foreign_main, int n_tables, int n_sets, int64_t n_calls, const int32_t *calls, int64_t *out)
{
    if (n_tables < 0 || n_sets < 0 || n_tables > 64 || n_sets > 64 || n_calls < 0) return -1;
    spl_lanes L;
    spl_lanes_init(&L, two, tail, foreign_main);
    spl_lane_table tables[64];
    spl_lane_set sets[64];
    for (int k = 0; k < 64; ++k) { spl_lane_table_init(&tables[k]); spl_lane_set_init(&sets[k]); }
    const int64_t stride = 6 + 4 * SPL_LANE_MAX_OPS;
    for (int64_t i = 0; i < n_calls; ++i) {
        const int32_t kind = calls[4 * i], a = calls[4 * i + 1], b = calls[4 * i + 2], c = calls[4 * i + 3];
        spl_lane_plan p = spl_lane_plan();
        if (kind == 0) { if (a < 0 || a >= n_sets) return -1; spl_lanes_relayout(&L, &sets[a], b, &p); }
        else if (kind == 1) { if (a < 0 || a >= n_tables || b < 0 || b >= n_sets) return -1; spl_lanes_count(&L, &tables[a], &sets[b], c, &p); }
        else if (kind == 2) spl_lanes_barrier(&L, &p);
        else if (kind == 3) { spl_lanes_join(&L, &p); spl_lanes_host_synced(&L); }
        else if (kind == 4) spl_lanes_main_work(&L, a, &p);
        else return -1;
        if (p.n_ops > SPL_LANE_MAX_OPS) return -1;
        int64_t *o = out + i * stride;
        o[0] = p.lane; o[1] = p.piped; o[2] = p.n_ops; o[3] = p.n_after; o[4] = p.n_mid; o[5] = p.tail_stream;
        for (int k = 0; k < p.n_ops; ++k) { o[6 + 4 * k] = p.ops[k].op; o[7 + 4 * k] = p.ops[k].stream; o[8 + 4 * k] = p.ops[k].kind; o[9 + 4 * k] = (int64_t)p.ops[k].seq; }
    }
    return 0;
}
#endif
