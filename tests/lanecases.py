"""The lanes of the counting passes without a GPU: a restatement of the rule of ``csrc/spl_lanes.h`` (``Lanes``: which stream a call
takes and which recorded events it waits for), a hazard checker that knows nothing of the rule (``check``: from a call sequence and a
plan it builds the happens-before graph -- stream order, the waits, the host's waits -- and asserts that every conflicting pair of
launches is ordered in launch order and that a barrier is one), and the call sequences the tests run (``SEQUENCES``, ``random_calls``).

A call is ``(kind, a, b, c)``: 0 relayout(set a, fused b); 1 count(table a, set b, piped c); 2 barrier; 3 download(table a); 4 other
work on the main stream (a: behind a join).  A plan entry is ``dict(lane, piped, n_after, n_mid, tail_stream, ops)`` -- the last
``n_after`` ops stand behind the call's launches, the ``n_mid`` before them between the range kernel and the tail -- and an op is
``(op, stream, kind, seq)``: op 1 wait / 2 record; stream 0 main, 1 second lane, 2 tail; kind 1 a pass's range kernel, 2 a tail on the
tail stream, 3 / 4 a marker on the main stream / the second lane, 5 a tail on the second lane."""
import random

RELAYOUT, COUNT, BARRIER, DOWNLOAD, MAIN_WORK = range(5)
MAIN, SIDE, TAIL = 0, 1, 2
NONE, EV_RANGE, EV_TAIL, EV_MAIN, EV_SIDE, EV_STAIL = range(6)
WAIT, RECORD = 1, 2
RING, MARKERS = 8, 4          # events the context keeps: per pass (range, tail), per kind of marker


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------
class Ev(object):
    def __init__(self, kind=NONE, seq=0, at=(0, 0, 0), via=0):
        self.kind, self.seq, self.at, self.via = kind, seq, tuple(at), via


def covered(a, by):
    return all(x <= y for x, y in zip(a, by))


def absorb(into, a):
    return [max(x, y) for x, y in zip(into, a)]


class Lanes(object):
    def __init__(self, two=True, tail=True, foreign_main=False):
        self.tail = bool(tail)
        self.two = bool(two) and self.tail
        self.foreign = bool(foreign_main)
        self.now = [[0, 0, 0] for _ in range(3)]
        self.side_floor = (0, 0, 0)
        self.tail_new, self.stail_new, self.main_ev, self.side_ev, self.floor_tail = Ev(), Ev(), Ev(), Ev(), Ev()
        self.n_pass = self.n_tail = self.n_stail = self.n_main = self.n_side = 0
        self.range_lane, self.range_set = 0, None
        self.tables, self.sets = {}, {}

    def table(self, k):
        return self.tables.setdefault(k, dict(range=Ev(), tail_prev=Ev(), tail_last=Ev()))

    def set(self, k):
        return self.sets.setdefault(k, dict(tail_prev=Ev(), tail_last=Ev(), lane=0, pending=False))

    def _wait(self, ops, stream, ev):
        if ev.kind == NONE or covered(ev.at, self.now[stream]):
            return
        if ev.kind == EV_RANGE and ev.seq + RING <= self.n_pass:
            ev = self.stail_new if ev.via == EV_STAIL else self.tail_new
        if ev.kind == EV_TAIL and ev.seq + RING <= self.n_tail:
            ev = self.tail_new
        if ev.kind == EV_STAIL and ev.seq + RING <= self.n_stail:
            ev = self.stail_new
        if ev.kind == EV_MAIN:
            ev = self.main_ev
        if ev.kind == EV_SIDE:
            ev = self.side_ev
        ops.append((WAIT, stream, ev.kind, ev.seq))
        self.now[stream] = absorb(self.now[stream], ev.at)

    def _record_main(self, ops):
        self.main_ev = Ev(EV_MAIN, self.main_ev.seq, self.now[MAIN])
        if not self.two:
            return
        self.n_main += 1
        self.main_ev.seq = self.n_main
        ops.append((RECORD, MAIN, EV_MAIN, self.n_main))

    def _join(self, ops):
        if not self.tail:
            return
        self._wait(ops, MAIN, self.tail_new)
        if self.now[SIDE][SIDE] > self.now[MAIN][SIDE]:
            self._wait(ops, MAIN, self.stail_new)
        if self.now[SIDE][SIDE] > self.now[MAIN][SIDE]:
            self.n_side += 1
            self.side_ev = Ev(EV_SIDE, self.n_side, self.now[SIDE])
            ops.append((RECORD, SIDE, EV_SIDE, self.n_side))
            self._wait(ops, MAIN, self.side_ev)

    def _settle(self, ops, lane):
        if lane != SIDE or covered(self.side_floor, self.now[SIDE]):
            return
        self._wait(ops, SIDE, self.floor_tail)
        if not covered(self.side_floor, self.now[SIDE]):
            if self.main_ev.kind == NONE or not covered(self.side_floor, absorb(self.now[SIDE], self.main_ev.at)):
                self._record_main(ops)
            self._wait(ops, SIDE, self.main_ev)

    def _floor(self):
        self.side_floor = tuple(self.now[MAIN])
        self.floor_tail = self.tail_new

    def call(self, kind, a=0, b=0, c=0):
        ops = []
        plan = dict(lane=0, piped=0, n_after=0, n_mid=0, tail_stream=0, ops=ops)
        if kind == RELAYOUT:
            s = self.set(a)
            lane = MAIN
            if self.two and b:
                if s["pending"] or self.range_set == a:
                    lane = s["lane"]
                elif self.range_set is not None:
                    lane = 1 - self.range_lane
            plan["lane"] = lane
            if self.tail:
                self._settle(ops, lane)
                self._wait(ops, lane, s["tail_last"])
                self.now[lane][lane] += 1
                s["lane"], s["pending"] = lane, True
        elif kind == COUNT and self.tail:
            t, s = self.table(a), self.set(b)
            if not c:
                self._join(ops)
                self.now[MAIN][MAIN] += 1
                before = len(ops)
                self._record_main(ops)
                plan["n_after"] = len(ops) - before
                self._floor()
                t["range"] = t["tail_prev"] = t["tail_last"] = s["tail_prev"] = s["tail_last"] = self.main_ev
                s["lane"], s["pending"] = MAIN, False
                self.range_lane, self.range_set = MAIN, b
            else:
                lane = s["lane"] if self.two else MAIN
                plan["lane"], plan["piped"] = lane, 1
                self._settle(ops, lane)
                self._wait(ops, lane, t["range"])
                self._wait(ops, lane, t["tail_prev"])
                self._wait(ops, lane, s["tail_prev"])
                self.now[lane][lane] += 1
                ts = SIDE if lane == SIDE else TAIL
                r = Ev(EV_RANGE, self.n_pass, self.now[lane], EV_STAIL if ts == SIDE else EV_TAIL)
                if ts == TAIL:
                    self.now[TAIL] = absorb(self.now[TAIL], r.at)
                head = len(ops)
                self._wait(ops, ts, t["tail_last"])
                self._wait(ops, ts, s["tail_last"])
                plan["n_mid"], plan["tail_stream"] = len(ops) - head, ts
                self.now[ts][ts] += 1
                if ts == SIDE:
                    tl = Ev(EV_STAIL, self.n_stail, self.now[ts])
                    self.n_stail += 1
                else:
                    tl = Ev(EV_TAIL, self.n_tail, self.now[ts])
                    self.n_tail += 1
                t["range"], t["tail_prev"], t["tail_last"] = r, t["tail_last"], tl
                s["tail_prev"], s["tail_last"], s["pending"] = s["tail_last"], tl, False
                if ts == SIDE:
                    self.stail_new = tl
                else:
                    self.tail_new = tl
                self.range_lane, self.range_set = lane, b
                self.n_pass += 1
        elif kind == BARRIER and self.tail:
            self._join(ops)
            if self.two:
                if self.foreign:
                    self.now[MAIN][MAIN] += 1
                self._floor()
                if not covered(self.side_floor, absorb(absorb(self.now[SIDE], self.tail_new.at), self.main_ev.at)):
                    self._record_main(ops)
        elif kind == DOWNLOAD:
            self._join(ops)
            top = [max(col) for col in zip(*self.now)]
            self.now = [list(top) for _ in range(3)]
        elif kind == MAIN_WORK and self.tail:
            if a:
                self._join(ops)
            self.now[MAIN][MAIN] += 1
            self._floor()
        return plan


def restated_plan(calls, two=True, tail=True, foreign_main=False):
    rule = Lanes(two, tail, foreign_main)
    return [rule.call(*c) for c in calls]


# ---- the checker ----------------------------------------------------------------------------------------------------------------
class Graph(object):
    """Launches, waits and records as nodes in launch order; anc[n]: the nodes that are over before n starts, as a bit set."""

    def __init__(self):
        self.anc, self.last, self.kernels = [], {}, []

    def node(self, stream, extra=(), kernel=None):
        n = len(self.anc)
        preds = list(extra) + ([self.last[stream]] if stream in self.last else [])
        bits = 0
        for p in preds:
            bits |= self.anc[p] | (1 << p)
        self.anc.append(bits)
        self.last[stream] = n
        if kernel is not None:
            self.kernels.append((n, kernel))
        return n

    def before(self, a, b):
        return bool(self.anc[b] >> a & 1)


def check(calls, plan, tail=True):
    """Asserts the hazards of the module's docstring for `calls` run by `plan`.  Returns the graph and, per call, its kernels' nodes."""
    g = Graph()
    recorded = {}                               # an event's handle -> the node of its latest record
    touched = {}                                # resource -> [(node, writes)]
    n_pass, n_tails, per_table, per_set = 0, {TAIL: 0, SIDE: 0}, {}, {}
    out = []

    def handle(kind, seq):
        return (kind, seq % (RING if kind in (EV_RANGE, EV_TAIL, EV_STAIL) else MARKERS))

    def run(ops):
        for op, stream, kind, seq in ops:
            if op == WAIT:
                assert handle(kind, seq) in recorded, "a wait for an event nobody recorded: %r" % ((kind, seq),)
                g.node(stream, [recorded[handle(kind, seq)]])
            else:
                assert op == RECORD
                recorded[handle(kind, seq)] = g.node(stream)

    def touch(n, resource, writes):
        for m, w in touched.setdefault(resource, []):
            if w or writes:
                assert g.before(m, n), "launches %d and %d both use %r and are not ordered" % (m, n, resource)
        touched[resource].append((n, writes))

    def everything_before(n, upto):
        for m, what in g.kernels:
            if m < upto:
                assert g.before(m, n), "%r (node %d) is not over before node %d" % (what, m, n)

    barrier_at = None
    first_after = set()
    for (kind, a, b, c), p in zip(calls, plan):
        nodes = {}
        ops = p["ops"]
        head = ops[:len(ops) - p["n_after"] - p["n_mid"]]
        mid = ops[len(head):len(ops) - p["n_after"]]
        if kind == RELAYOUT:
            run(head)
            n = nodes["slots"] = g.node(p["lane"], kernel=("slots", a))
            touch(n, ("slots", a), True)
        elif kind == COUNT:
            run(head)
            k = per_table.get(a, 0)
            q = per_set.get(b, 0)
            per_table[a], per_set[b] = k + 1, q + 1
            if p["piped"]:
                assert tail
                n = nodes["range"] = g.node(p["lane"], kernel=("range", a, b))
                touch(n, ("table", a), True)
                touch(n, ("copy", a, k % 3), True)
                touch(n, ("slots", b), False)
                touch(n, ("queue", b, q % 2), True)
                recorded[handle(EV_RANGE, n_pass)] = r = g.node(p["lane"])
                ts = p["tail_stream"]
                assert ts == (SIDE if p["lane"] == SIDE else TAIL)
                if ts == TAIL:
                    g.node(TAIL, [r])
                run(mid)
                n = nodes["tail"] = g.node(ts, kernel=("tail", a, b))
                touch(n, ("scan outputs", a), True)                # (the tails on one table share them)
                touch(n, ("copy", a, k % 3), True)
                touch(n, ("copy", a, (k + 2) % 3), True)       # (the copy it clears for the pass after next)
                touch(n, ("slots", b), False)
                touch(n, ("queue", b, q % 2), False)
                recorded[handle(EV_STAIL if ts == SIDE else EV_TAIL, n_tails[ts])] = g.node(ts)
                n_tails[ts] += 1
                n_pass += 1
            else:                                               # everything on the main stream: range / pair kernel, tail, a layout
                assert p["lane"] == MAIN
                n = nodes["range"] = nodes["tail"] = g.node(MAIN, kernel=("serial pass", a, b))
                if tail:
                    everything_before(n, n)
                for resource in [("table", a), ("slots", b), ("scan outputs", a)] + [("copy", a, j) for j in range(3)] + [("queue", b, j) for j in range(2)]:
                    touch(n, resource, True)
        elif kind == BARRIER:
            run(head)
            barrier_at, first_after = len(g.anc), set()
        elif kind == DOWNLOAD:
            run(head)
            n = nodes["download"] = g.node(MAIN, kernel=("download", a))
            everything_before(n, n)
            for s in (MAIN, SIDE, TAIL):                        # (the host has waited: whatever comes next comes after it)
                g.last[s] = n
        elif kind == MAIN_WORK:
            run(head)
            n = nodes["work"] = g.node(MAIN, kernel=("work",))
            if a:
                everything_before(n, n)
        run(ops[len(ops) - p["n_after"]:])
        if barrier_at is not None:
            for n in nodes.values():
                everything_before(n, barrier_at)
        out.append(nodes)
    return g, out


# ---- sequences ------------------------------------------------------------------------------------------------------------------
def bench_steps(n_shards, n_steps, barriers=True, relayout=True):
    calls = []
    for _ in range(n_steps):
        for k in range(n_shards):
            if relayout:
                calls.append((RELAYOUT, k, 1, 0))
            calls.append((COUNT, k, k, 1))
        if barriers:
            calls.append((BARRIER, 0, 0, 0))
    return calls


def _turns(pairs, n, relayout):
    calls = []
    for i in range(n):
        t, s = pairs[i % len(pairs)]
        if relayout:
            calls.append((RELAYOUT, s, 1, 0))
        calls.append((COUNT, t, s, 1))
    return calls


SEQUENCES = {}
for shards in (1, 2, 3):
    SEQUENCES["bench %d shards" % shards] = bench_steps(shards, 6)
    SEQUENCES["bench %d shards, no barriers" % shards] = bench_steps(shards, 6, barriers=False)
    SEQUENCES["bench %d shards, no relayout" % shards] = bench_steps(shards, 6, barriers=False, relayout=False)
SEQUENCES["one table, two sets taking turns"] = _turns([(0, 0), (0, 1)], 12, True)
SEQUENCES["one table, two sets taking turns, no relayout"] = _turns([(0, 0), (0, 1)], 12, False)
SEQUENCES["one set, two tables taking turns"] = _turns([(0, 0), (1, 0)], 12, True)
SEQUENCES["one set, two tables taking turns, no relayout"] = _turns([(0, 0), (1, 0)], 12, False)
SEQUENCES["a pair-kernel pass in between"] = (bench_steps(2, 2) + [(COUNT, 0, 0, 0), (COUNT, 0, 0, 0), (RELAYOUT, 1, 1, 0), (COUNT, 1, 1, 1), (RELAYOUT, 0, 0, 0), (COUNT, 0, 0, 1)]
                                              + bench_steps(2, 2, barriers=False) + [(COUNT, 1, 1, 0)] + bench_steps(2, 2))
SEQUENCES["a download between two passes"] = [(RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1), (RELAYOUT, 1, 1, 0), (COUNT, 1, 1, 1), (DOWNLOAD, 0, 0, 0), (RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1),
                                              (DOWNLOAD, 1, 0, 0), (RELAYOUT, 1, 1, 0), (COUNT, 1, 1, 1), (DOWNLOAD, 1, 0, 0), (DOWNLOAD, 0, 0, 0)]
SEQUENCES["a slots kernel no pass follows, then a barrier"] = [(RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1), (RELAYOUT, 1, 1, 0), (BARRIER, 0, 0, 0), (RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1),
                                                               (RELAYOUT, 1, 1, 0), (COUNT, 1, 1, 1), (MAIN_WORK, 1, 0, 0), (RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1)]
SEQUENCES["a new set's first layout, then the second lane"] = [(RELAYOUT, 0, 1, 0), (COUNT, 0, 0, 1), (MAIN_WORK, 0, 0, 0), (RELAYOUT, 1, 1, 0), (COUNT, 1, 1, 1), (BARRIER, 0, 0, 0),
                                                               (MAIN_WORK, 0, 0, 0), (COUNT, 0, 2, 1), (RELAYOUT, 2, 1, 0), (COUNT, 0, 2, 1)]
SEQUENCES["many sets over one table"] = [c for i in range(40) for c in ((RELAYOUT, i % 11, 1, 0), (COUNT, 0, i % 11, 1))]


def random_calls(seed, n=40, n_tables=3, n_sets=4):
    rng = random.Random(seed)
    fused = [rng.random() < 0.85 for _ in range(n_sets)]
    calls = []
    for _ in range(n):
        r = rng.random()
        if r < 0.35:
            k = rng.randrange(n_sets)
            calls.append((RELAYOUT, k, int(fused[k]), 0))
        elif r < 0.80:
            calls.append((COUNT, rng.randrange(n_tables), rng.randrange(n_sets), int(rng.random() < 0.9)))
        elif r < 0.88:
            calls.append((BARRIER, 0, 0, 0))
        elif r < 0.94:
            calls.append((DOWNLOAD, rng.randrange(n_tables), 0, 0))
        else:
            calls.append((MAIN_WORK, int(rng.random() < 0.7), 0, 0))
    return calls
