"""Pure-Python restatement of the witness cycle of include/maelsim.h (msim_cycle_result / msim_cycle_step) — written independently of
csrc/txn_check.cpp and csrc/cycle_classify.inc: the merged edge map of a history in tests/elle_ref.py's dict / set style (list-append
and rw-register), the class by plain reachability, the witness by plain BFS straight from the definition, and verify(), which checks
a reported cycle against the edge map alone.  Test infrastructure only.

history: list of op maps {type, process, value=[[f, k, v], ...]}, one per row (as engine.encode_txn_history lays them out)."""
WW, WR, RW, RT = 1, 2, 4, 8
G0, G1C, G_SINGLE, G2, REALTIME = 1, 8, 16, 32, 512
NO_VALUE = 0xFFFFFFFF


def _transactions(ops):
    """[{id, type, mops, inv, cmp}] and the realtime predecessors (the frontier at the invocation, transitively reduced)"""
    txns, open_by_proc, frontier, rt_pred = [], {}, [], {}
    for i, op in enumerate(ops):
        if op.get("process") == ":nemesis" or op.get("f") != ":txn":
            continue
        p = op["process"]
        if op["type"] == ":invoke":
            t = {"id": len(txns), "type": ":info", "mops": op["value"], "inv": i, "cmp": NO_VALUE}
            open_by_proc[p] = t
            rt_pred[t["id"]] = list(frontier)
            txns.append(t)
        elif open_by_proc.get(p) is not None:
            t = open_by_proc.pop(p)
            t["type"], t["cmp"] = op["type"], i
            if op["type"] == ":ok":
                t["mops"] = op["value"]
                frontier = [f for f in frontier if f not in rt_pred[t["id"]]] + [t["id"]]
    return txns, rt_pred


def _realtime(txns, rt_pred, add):
    for t in txns:
        if t["type"] != ":fail":
            for f in rt_pred[t["id"]]:
                add(f, t["id"], RT)


def edges_list_append(ops):
    """(transactions, {(a, b): kinds}) of a list-append history: ww along each key's longest read, wr / rw per compatible read, realtime"""
    txns, rt_pred = _transactions(ops)
    writer = {}
    for t in txns:
        for f, k, v in t["mops"]:
            if f == ":append":
                writer[(k, v)] = t["id"]
    longest = {}
    for t in txns:
        if t["type"] == ":ok":
            for f, k, v in t["mops"]:
                if f == ":r" and (k not in longest or len(v or []) > len(longest[k])):
                    longest[k] = list(v or [])
    edges = {}

    def add(a, b, kind):
        if a != b:
            edges[(a, b)] = edges.get((a, b), 0) | kind
    live = lambda w: w is not None and txns[w]["type"] != ":fail"
    for k, order in longest.items():
        for x, y in zip(order, order[1:]):
            a, b = writer.get((k, x)), writer.get((k, y))
            if live(a) and live(b):
                add(a, b, WW)
    for t in txns:
        if t["type"] != ":ok":
            continue
        for f, k, v in t["mops"]:
            if f != ":r" or k not in longest:
                continue
            lst, order = v or [], longest[k]
            if lst != order[:len(lst)]:
                continue
            ext = list(lst)
            while ext and writer.get((k, ext[-1])) == t["id"]:
                ext.pop()
            if ext and live(writer.get((k, ext[-1]))):
                add(writer[(k, ext[-1])], t["id"], WR)
            if len(lst) < len(order) and live(writer.get((k, order[len(lst)]))):
                add(t["id"], writer[(k, order[len(lst)])], RW)
    _realtime(txns, rt_pred, add)
    return txns, edges


def edges_rw(ops):
    """the same of a rw-register history: version orders from the initial nil and writes that follow reads (tests/elle_ref.py analyse_rw)"""
    txns, rt_pred = _transactions(ops)
    writer, final = {}, {}
    for t in txns:
        for f, k, v in t["mops"]:
            if f == ":w":
                writer[(k, v)] = t["id"]
                final[(t["id"], k)] = v
    live = lambda w: w is not None and txns[w]["type"] != ":fail"
    edges = {}

    def add(a, b, kind):
        if a != b:
            edges[(a, b)] = edges.get((a, b), 0) | kind
    succ, versions, ext_reads = {}, {}, []
    for t in txns:
        if t["type"] != ":fail":
            for f, k, v in t["mops"]:
                if f == ":w":
                    versions.setdefault(k, set()).add(v)
        if t["type"] != ":ok":
            continue
        state = {}
        for f, k, v in t["mops"]:
            if f == ":w":
                state[k] = v
                continue
            if k in state:
                continue
            state[k] = v
            ext_reads.append((t["id"], k, v))
            if v is None:
                continue
            versions.setdefault(k, set()).add(v)
            w = writer.get((k, v))
            if not live(w):
                continue
            if w != t["id"]:
                add(w, t["id"], WR)
            fw = final.get((t["id"], k))
            if fw is not None and fw != v:
                succ.setdefault(k, {}).setdefault(v, set()).add(fw)
    for k, vs in versions.items():
        succ.setdefault(k, {}).setdefault(None, set()).update(vs)
    for k in list(succ):
        g = succ[k]

        def reach(a):
            seen, stack = set(), [a]
            while stack:
                for b in g.get(stack.pop(), ()):
                    if b not in seen:
                        seen.add(b)
                        stack.append(b)
            return seen
        if any(v in reach(v) for v in list(g)):
            succ[k] = {}
            continue
        for v1, v2s in g.items():
            for v2 in v2s:
                if v1 is not None and live(writer.get((k, v1))) and live(writer.get((k, v2))):
                    add(writer[(k, v1)], writer[(k, v2)], WW)
    for tid, k, v in ext_reads:
        for v2 in succ.get(k, {}).get(v, ()):
            if live(writer.get((k, v2))):
                add(tid, writer[(k, v2)], RW)
    _realtime(txns, rt_pred, add)
    return txns, edges


def _adj(edges, mask):
    adj = {}
    for (a, b), ks in edges.items():
        if ks & mask:
            adj.setdefault(a, []).append(b)
    return adj


def _bfs(adj, src):
    d, level = {src: 0}, [src]
    while level:
        nxt = []
        for v in level:
            for w in adj.get(v, ()):
                if w not in d:
                    d[w] = d[v] + 1
                    nxt.append(w)
        level = nxt
    return d


def _on_cycle(adj, t):
    return any(t in _bfs(adj, w) for w in adj.get(t, ()))


def classify(edges):
    """(class bit, x) as the analysis names them: the dependency edges alone first, the lowest class; (0, 0): no cycle"""
    for x in (0, RT):
        for cls, mask in ((G0, WW), (G1C, WW | WR), (G2, WW | WR | RW)):
            adj = _adj(edges, mask | x)
            if any(_on_cycle(adj, t) for t in adj):
                if cls == G2:
                    nadj = _adj(edges, WW | WR | x)
                    if any(ks & RW and u in _bfs(nadj, v) for (u, v), ks in edges.items()):
                        cls = G_SINGLE
                return cls, x
    return 0, 0


def witness(edges):
    """(anomaly bits, [(transaction, kinds of the step to the next)]) by the definition; (0, []) if there is no cycle"""
    cls, x = classify(edges)
    if not cls:
        return 0, []
    bits = cls | (REALTIME if x else 0)
    if cls == G_SINGLE:
        n_mask = WW | WR | x
        adj = _adj(edges, n_mask)
        for v0 in sorted({v for (u, v), ks in edges.items() if ks & RW}):
            d = _bfs(adj, v0)
            tails = [(d[u], u) for (u, v), ks in edges.items() if v == v0 and ks & RW and u in d]
            if tails:
                break
        mask, (L, u) = n_mask, min(tails)
        start = v0
    else:
        mask = {G0: WW, G1C: WW | WR, G2: WW | WR | RW}[cls] | x
        adj = _adj(edges, mask)
        start = min(t for t in adj if _on_cycle(adj, t))
        d = _bfs(adj, start)
        L, u = min((d[a], a) for (a, b), ks in edges.items() if b == start and ks & mask and a in d)
    path = [u]
    for i in range(L, 0, -1):
        path.append(min(w for (w, b), ks in edges.items() if b == path[-1] and ks & mask and d.get(w) == i - 1))
    path.reverse()
    assert path[0] == start
    cycle = [(a, edges[(a, b)] & mask) for a, b in zip(path, path[1:])]
    cycle.append((u, RW if cls == G_SINGLE else edges[(u, start)] & mask))
    return bits, cycle


def verify(edges, bits, cycle):
    """a reported cycle [(transaction, kinds)] against the edge map alone: every step is an edge of exactly the stated kinds, the cycle
    closes, the class constraint holds, and no shorter cycle through step 0 exists over the mask"""
    cls, x = bits & (G0 | G1C | G_SINGLE | G2), (RT if bits & REALTIME else 0)
    assert cls in (G0, G1C, G_SINGLE, G2) and cycle
    mask = {G0: WW, G1C: WW | WR, G_SINGLE: WW | WR, G2: WW | WR | RW}[cls] | x
    n = len(cycle)
    assert len({t for t, _ in cycle}) == n, "a transaction twice"
    for i, (a, kinds) in enumerate(cycle):
        b = cycle[(i + 1) % n][0]          # (the last step returns to step 0: the cycle closes)
        assert (a, b) in edges and kinds, (i, a, b)
        if cls == G_SINGLE and i == n - 1:
            assert kinds == RW and edges[(a, b)] & RW, (i, a, b, kinds)
        else:
            assert kinds == edges[(a, b)] & mask, (i, a, b, kinds, edges[(a, b)])
    rw_steps = [i for i, (_, k) in enumerate(cycle) if k & RW]
    if cls in (G0, G1C):
        assert not rw_steps
    if cls == G0:
        assert all(k & ~(WW | x) == 0 for _, k in cycle)
    if cls == G_SINGLE:
        assert rw_steps == [n - 1]
    if x:
        assert classify({e: k & ~RT for e, k in edges.items() if k & ~RT})[0] == 0, "a cycle without realtime edges exists"
    # the shortest: over the mask no path from step 0 reaches a closing transaction in fewer steps
    start = cycle[0][0]
    d = _bfs(_adj(edges, mask), start)
    close = RW if cls == G_SINGLE else mask
    assert min(d[a] for (a, b), ks in edges.items() if b == start and ks & close and a in d) == n - 1
    return True
