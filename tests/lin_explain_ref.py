"""Pure-Python explaining linearizability search over binary lin-kv rows: the record msim_explain_lin_kv_rows writes per key
(include/maelsim.h msim_lin_key_result), from a search WITHOUT dominance or symmetry pruning, in the style of tests/linearizable_ref.py.
TEST INFRASTRUCTURE.

Per key: Knossos' :op (the row of the first :ok completion whose return leaves no configuration), :previous-ok (the row of the last :ok
completion that returned before it), the register values over the configurations just before that op (or the ones the key ends with)
and the calls open at that moment.  Odd rows as csrc/lin_check.cpp takes them: a completion without an open invocation of its process
is ignored, a second invocation of an open process replaces the first (which then never completes)."""
NO_VALUE = 0xFFFFFFFF
T_INVOKE, T_OK, T_FAIL, T_INFO = range(4)
F_READ, F_WRITE, F_CAS = 2, 6, 7
NEMESIS = 0xFFFFF
NIL = 0xFF


def _record(key, valid, op_row, prev_ok, n_pending, values):
    vs = sorted(values)   # nil = 0xFF is the largest: last
    return {"key": key, "valid": valid, "op_row": op_row, "previous_ok_row": prev_ok, "n_pending": n_pending, "n_values": len(vs),
            "values": (vs[:8] + [0] * 8)[:8]}


def explain_key(key, ops):
    """ops: [(row index, type, f, process, v1, v2)] of one key, in order."""
    open_by_proc, comp = {}, {}
    for i, (_, typ, _, proc, _, _) in enumerate(ops):
        if typ == T_INVOKE:
            open_by_proc[proc] = i
        elif proc in open_by_proc:
            comp[open_by_proc.pop(proc)] = i
    inv_of = {c: i for i, c in comp.items()}
    events, eff = [], {}
    for i, (row, typ, f, proc, v1, v2) in enumerate(ops):
        if typ == T_INVOKE:
            c = comp.get(i)
            if c is not None and ops[c][1] == T_FAIL:
                continue                                   # never happened
            ok = c is not None and ops[c][1] == T_OK
            src = ops[c] if ok else ops[i]                 # an :ok read carries the value it saw
            eff[i] = {"f": f, "v1": src[4], "v2": src[5], "skip": (not ok) and f == F_READ}
            events.append(("call", i, row))
        elif typ == T_OK and i in inv_of and inv_of[i] in eff:
            events.append(("ret", inv_of[i], row))

    def step(state, e):
        if e["f"] == F_READ:
            return state == e["v1"], state
        if e["f"] == F_WRITE:
            return True, e["v1"]
        return state == e["v1"], e["v2"]

    def open_calls():
        return sum(1 for j in pending if not eff[j]["skip"])

    configs = {(NIL, frozenset())}
    pending = set()
    prev_ok = NO_VALUE
    for kind, i, row in events:
        if kind == "call":
            if len(pending) == 64:                         # the searches hold 64 open calls of a key
                return _record(key, 2, NO_VALUE, NO_VALUE, 0, [])
            pending.add(i)
            continue
        before = {st for st, _ in configs}
        out, seen, stack = set(), set(configs), list(configs)
        while stack:
            state, lin = stack.pop()
            if i in lin:
                out.add((state, lin - {i}))
                continue
            for j in pending - lin:
                if eff[j]["skip"]:
                    continue
                ok, st2 = step(state, eff[j])
                if ok:
                    c2 = (st2, lin | {j})
                    if c2 not in seen:
                        seen.add(c2)
                        stack.append(c2)
        pending.discard(i)
        if not out:
            return _record(key, 0, row, prev_ok, open_calls(), before)
        configs = out
        prev_ok = row
    return _record(key, 1, NO_VALUE, NO_VALUE, open_calls(), {st for st, _ in configs})


def explain(rows):
    """rows: the binary history (numpy OP_DT records) -> the key records, ascending by key."""
    by_key = {}
    for idx in range(len(rows)):
        packed, value = int(rows["packed"][idx]), int(rows["value"][idx])
        typ, f, proc = packed & 3, (packed >> 2) & 31, packed >> 12
        if proc == NEMESIS or f not in (F_READ, F_WRITE, F_CAS):
            continue
        by_key.setdefault(value & 0xFF, []).append((idx, typ, f, proc, (value >> 8) & 0xFF, (value >> 16) & 0xFF))
    return [explain_key(k, by_key[k]) for k in sorted(by_key)]
