#!/usr/bin/env python3
"""Developer tool (CPU only): what pairing the op rounds of the duo kernel's two clusters (csrc/duo.hip, "PAIRED OP ROUNDS") saves, from
the oracle's histories and a replay model of the wavefront's rounds.

The ops of N instances of a latency-0 broadcast configuration are taken from the oracle's rows (the invocation rows: function and node).
The round model: a read is 1 cluster round; a broadcast at node v is ecc(v) + 2 cluster rounds (the op's round, ecc(v) rounds until the
farthest node has the value, one more until its last duplicates are handled), ecc = the node's eccentricity in the topology.  The model
is checked against the oracle's n_rounds first (printed: the rounds it does not explain, per instance and per broadcast).

The replay pairs the instances (2k, 2k + 1) as the kernel's wavefronts do.  A cluster is in a flood (g gossip rounds to go) or ready for
its next op; a read rides in the run of the op behind it unless it is the last draw of a block of 32 or the cluster's last op.  Every
wave-round, a ready cluster takes its op round ("today"), or waits for a partner in mid-flood for up to CAP wave-rounds and takes it
together with the partner's, or alone when the wait runs out ("paired").  Cycles use the costs measured for the round bodies
(profiles/r12_round_split_after.txt): an op wave-round 758 + 1989 + 1115 per read of the longest run among the acting halves, a gossip
round 555, a parked gossip round PARKED_CYCLES.

    python tools/duo_pair_estimate.py [--n 16] [--first 0] [--seed 2026] [--cap 24] [--nodes 25] [--topology grid] [--time-limit 20] [--rate 100]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OP_BASE, OP_PER_READ, GOSSIP = 758 + 1989, 1115, 555


def eccentricities(topology, n):
    side = 1
    while side * side < n:
        side += 1
    adj = []
    for a in range(n):
        if topology == "grid":
            i, j = divmod(a, side)
            nb = [a + 1] * (j + 1 < side and a + 1 < n) + [a - 1] * (j > 0) + [a + side] * (a + side < n) + [a - side] * (i > 0)
        elif topology == "line":
            nb = [a + 1] * (a + 1 < n) + [a - 1] * (a > 0)
        elif topology == "total":
            nb = [b for b in range(n) if b != a]
        else:
            raise SystemExit(f"topology {topology}: grid, line or total")
        adj.append(nb)
    ecc = []
    for a in range(n):
        dist, frontier = {a: 0}, [a]
        while frontier:
            nxt = []
            for u in frontier:
                for v in adj[u]:
                    if v not in dist:
                        dist[v] = dist[u] + 1
                        nxt.append(v)
            frontier = nxt
        ecc.append(max(dist.values()))
    return ecc


def cluster_ops(rows):
    """[(is_read, node)] of the generator's ops, in order (the final reads are not the generator's)"""
    r = np.frombuffer(rows.tobytes(), dtype=np.uint32).reshape(-1, 4)
    ops = []
    for w in r[:, 2]:
        w = int(w)
        if (w & 3) == 0 and not (w >> 11) & 1:
            ops.append((((w >> 2) & 0x1FF) == 2, w >> 12))
    return ops


def events(ops, ecc):
    """the cluster's op rounds: (reads that ran ahead, gossip rounds of the flood behind the op)"""
    out, run = [], 0
    for k, (is_read, node) in enumerate(ops):
        if is_read and k % 32 != 31 and k + 1 < len(ops):
            run += 1
            continue
        out.append((run + (1 if is_read else 0), 0 if is_read else ecc[node] + 1))
        run = 0
    return out


def replay(ev_a, ev_b, cap, parked_cycles):
    """wave-rounds, op wave-rounds, op wave-rounds with two ops, parks, parked rounds, longest wait, cycles"""
    ev = [ev_a, ev_b]
    at, g = [0, 0], [0, 0]              # next event, gossip rounds to go
    waited = [0, 0]
    done = [not ev_a, not ev_b]
    n_wave = n_op = n_two = n_parks = n_parked = longest = cycles = 0
    while not all(done):
        ready = [not done[h] and g[h] == 0 for h in (0, 1)]
        act = list(ready)
        if cap and ready[0] != ready[1]:
            h = 0 if ready[0] else 1
            if not done[1 - h] and waited[h] < cap:   # the partner is in mid-flood: wait
                act[h] = False
                n_parks += waited[h] == 0
                waited[h] += 1
                n_parked += 1
                longest = max(longest, waited[h])
        n_wave += 1
        if any(act):
            n_op += 1
            n_two += all(act)
            reads = max(ev[h][at[h]][0] for h in (0, 1) if act[h])
            cycles += OP_BASE + OP_PER_READ * reads
        else:
            cycles += parked_cycles if (ready[0] or ready[1]) else GOSSIP
        for h in (0, 1):
            if act[h]:
                g[h] = ev[h][at[h]][1]
                at[h] += 1
                waited[h] = 0
                done[h] = at[h] == len(ev[h]) and g[h] == 0
            elif not done[h] and g[h] > 0:
                g[h] -= 1
                done[h] = at[h] == len(ev[h]) and g[h] == 0
    return np.array([n_wave, n_op, n_two, n_parks, n_parked, longest, cycles], dtype=np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--seed", type=int, default=2026)
    ap.add_argument("--cap", type=int, default=24)
    ap.add_argument("--nodes", type=int, default=25)
    ap.add_argument("--topology", default="grid")
    ap.add_argument("--time-limit", type=float, default=20)
    ap.add_argument("--rate", type=float, default=100)
    ap.add_argument("--parked-cycles", type=int, default=GOSSIP)
    a = ap.parse_args()
    from maelstrom_amd import engine as E
    import oracle_lib as O
    cfg = E.test_config(workload="broadcast", bin="broadcast-ff", node_count=a.nodes, rate=a.rate, time_limit=a.time_limit, latency=0, inbox_capacity=6, topology=a.topology, seed=a.seed)
    ora = O.run(cfg, a.first, a.n)
    ecc = eccentricities(a.topology, a.nodes)
    ops = [cluster_ops(ora.history(i)[0]) for i in range(a.n)]
    # the round model against the oracle
    model = np.array([sum(1 if rd else ecc[v] + 2 for rd, v in o) for o in ops], dtype=np.float64)
    real = np.array([int(ora.meta[i]["n_rounds"]) for i in range(a.n)], dtype=np.float64)
    nb = np.array([sum(1 for rd, _ in o if not rd) for o in ops], dtype=np.float64)
    print(f"{a.n} instances from {a.first}, seed {a.seed}, {a.topology} of {a.nodes} (eccentricities {min(ecc)} .. {max(ecc)}, mean {np.mean(ecc):.1f}): "
          f"ops per cluster {np.mean([len(o) for o in ops]):.0f}, broadcasts {nb.mean():.0f}")
    print(f"round model: read = 1, broadcast = ecc + 2: {model.mean():.0f} cluster rounds, the oracle's n_rounds {real.mean():.0f}; unexplained "
          f"{(real - model).mean():.1f} per instance, {100 * np.abs(real - model).max() / max(nb.mean(), 1):.2f} % of a round per broadcast at most")
    evs = [events(o, ecc) for o in ops]
    pairs = [(evs[k], evs[k + 1] if k + 1 < a.n else []) for k in range(0, a.n, 2)]
    for name, cap in (("today", 0), (f"paired, cap {a.cap}", a.cap)):
        t = np.mean([replay(x, y, cap, a.parked_cycles) for x, y in pairs], axis=0)
        longest = max(replay(x, y, cap, a.parked_cycles)[5] for x, y in pairs)
        print(f"{name:16s}: wave-rounds {t[0]:.0f}, with an op {t[1]:.0f} (two ops {t[2]:.0f}; {t[1] / max(2 * nb.mean(), 1):.2f} per broadcast), parks {t[3]:.0f}, "
              f"parked rounds {t[4]:.0f} (longest wait {longest:.0f}), modelled cycles {t[6]:.3e} per wavefront")


if __name__ == "__main__":
    main()
