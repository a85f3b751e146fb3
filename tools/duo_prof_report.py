#!/usr/bin/env python3
"""Developer tool (GPU box): runs the headline batch with the DUO_PROF build (tools/variant_lib.sh prof duo.hip -DDUO_PROF) and prints, per wavefront,
the number of wave-rounds, how many of them were GENERAL rounds (op rounds and full GENERAL bodies), and the cycles spent in each kind; then the
flood bodies (flood gossip rounds, flood op rounds) and the materialisations, which the wavefront's upper instance carries; and the
wave-rounds with an op, the ops they executed, and how many of those were reads that ran ahead of their wave-round's op (read runs); and
the paired op rounds: parks, parked gossip rounds per park and their cycles, the longest wait, op wave-rounds that carried one op or two.
And the quiet op rounds: how many of the flood op rounds took the body without the exchange.
TOPOLOGY / NODES choose another shape (e.g. TOPOLOGY=line NODES=24, the long floods the wait cap is for).
STRETCH=1: the library is a -DDUO_PROF -DDUO_PROF_STRETCH build (tools/variant_lib.sh profstretch duo.hip -DDUO_PROF -DDUO_PROF_STRETCH), whose lower
instance carries the flood stretches, the rounds taken inside them and the generic gossip rounds with their cycles, counted directly, in place of
the GENERAL bodies' and generic op rounds' figures: the lines about those are left out, the stretch lines are printed.
STEADY=1: the library is a -DDUO_PROF -DDUO_PROF_STEADY build (tools/variant_lib.sh profsteady duo.hip -DDUO_PROF -DDUO_PROF_STEADY), whose lower
instance carries the steady parks, the steady leaves and the cycles of both (from the stretch's exit to the re-entry of the stretch or the op
round's head) in place of the GENERAL bodies' and generic op rounds' cycles and the quiet count: the lines that need those are left out, and the
leaving rounds are split into fast ones (steady parks and leaves) and slow ones (through R0 and the exit test) with the cycles of each.
How to read that split: a slow round's cycles are counted from the loop's head, so where the steady leave looked and declined, the cycles between
the stretch's exit and the loop's head (the declined test) are in no bucket, and "slow at N cycles each" leaves them out; the fast cycles are a
10-bit field in units of 4096 per wavefront, read at the middle of its unit (+2048 per wavefront, a bias of at most that much either way).
The line "steady fields" says in how many wavefronts a field is saturated.  As of round 17 the -DDUO_PROF_STEADY build does not fit its SGPRs (139
spills, v_readlane / v_writelane inside the loops: profiles/r31_round_split_after.txt), so its counts are exact and its cycles are its own spills'.
(Both of those builds leave the flood memo out, see DUO_MEMO_ON in csrc/duo.hip: they count the rounds of simulated floods.)
MEMO=1: the library is a -DDUO_PROF -DDUO_PROF_MEMO build (tools/variant_lib.sh profmemo duo.hip -DDUO_PROF -DDUO_PROF_MEMO), in which BOTH instances of a
wavefront carry, in place of the cycles of the GENERAL bodies, generic op rounds, flood gossip rounds and leaving rounds and of the quiet count:
the floods their cluster replayed (16 bits), the broadcasts it took outside the quiet body (8 bits, saturating) and the floods the wavefront
recorded (8 bits); the upper instance's reserved[2] is the number of recordings the wavefront dropped.  Only counts are printed: wave-rounds, op wave-rounds, flood gossip and parked rounds, parks, recorded and replayed floods.
MEMO=1 RUN=1: the library is a -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN build (tools/variant_lib.sh profrun duo.hip -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN), whose lower
instance carries in reserved[2], in place of all cycles, the parks and the longest wait: the iterations of the runs' loop (16 bits) and the broadcasts of both
clusters taken in runs (16 bits), the steady run of csrc/duo.hip; those two figures are printed, the parks and the cycles are left out.
MEMO=1 RUN=1 PLAN=1: the library is that build with -DDUO_PROF_PLAN as well (tools/variant_lib.sh profplan duo.hip -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN -DDUO_PROF_PLAN),
whose upper instance carries in reserved[2], in place of the recordings dropped: the block plans that took an op (16 bits) and the ops they took (16 bits), the
block plan of csrc/duo.hip; printed with the ops the runs' loop still took (the runs' reads and broadcasts less the plans' ops).
(Every -DDUO_PROF build leaves the flood table out unless -DDUO_PROF_TABLE is given as well, see DUO_TABLE_ON in csrc/duo.hip: without it a wavefront records
its own floods, as the parent of round 21 did; with it, e.g. tools/variant_lib.sh profruntab duo.hip -DDUO_PROF -DDUO_PROF_MEMO -DDUO_PROF_RUN -DDUO_PROF_TABLE, "floods
recorded" counts what the wavefront still had to record itself.  The switches above read the same words either way.)
(Every -DDUO_PROF build WITHOUT -DDUO_PROF_RUN leaves the steady run out, see DUO_SRUN_ON in csrc/duo.hip: its figures split the op wave-rounds of the kernel
without the run by the body that took them; the counts of the kernel as it ships are those of the RUN=1 build.)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("MSIM_LIB", os.path.join(ROOT, "maelstrom_amd", "libmaelsim_prof.so"))
sys.path.insert(0, ROOT)
from maelstrom_amd import engine as E  # noqa: E402

kw = dict(workload="broadcast", bin="broadcast-ff", node_count=int(os.environ.get("NODES", "25")), rate=100, time_limit=20, latency=int(os.environ.get("LAT", "0")), latency_dist=os.environ.get("DIST", "constant"), seed=2026)
if kw["latency"] == 0:
    kw["inbox_capacity"] = 6
if os.environ.get("TOPOLOGY"):
    kw["topology"] = os.environ["TOPOLOGY"]
n = int(os.environ.get("N", "4096"))
cfg = E.test_config(**kw)
with E.Engine(cfg) as eng:
    eng.run(0, n)
    eng.run(n, n)
    sim_ms = eng.kernel_ms()[0]
    eng.fetch()
    m = np.array([[eng.meta(i).n_events, eng.meta(i).reserved[0], eng.meta(i).reserved[1], eng.meta(i).reserved[2], eng.meta(i).n_rounds] for i in range(0, n, 2)], dtype=np.float64)
    # the counts that share a word with the read-run counter have 16 bits each: a wavefront runs at most the rounds of its two clusters together
    assert 2 * max(eng.meta(i).n_rounds for i in range(n)) < 65536, "this shape runs too many rounds for the 16-bit fields of the DUO_PROF build"
    up = np.array([[eng.meta(i).n_events, eng.meta(i).reserved[0], eng.meta(i).reserved[1], eng.meta(i).reserved[2]] for i in range(1, n, 2)], dtype=np.int64)
ev, nwave, cyc, ctot, rounds = m.T
# the upper 16 bits of the wave-round count (lower instance): the reads of both clusters that a read run executed; of the flood gossip
# round count (upper instance): the parked gossip rounds; beside all cycles / 4096: the parks (11 bits) and the longest wait (5 bits)
nrun = (nwave.astype(np.int64) >> 16).astype(np.float64)
nwave = (nwave.astype(np.int64) & 0xFFFF).astype(np.float64)
npk = (up[:, 0] >> 16).astype(np.float64)
up[:, 0] &= 0xFFFF
run = os.environ.get("RUN", "0") != "0"
nit, nrunb = (ctot.astype(np.int64) & 0xFFFF).astype(np.float64), (ctot.astype(np.int64) >> 16).astype(np.float64)   # (RUN=1: what reserved[2] of the lower instance holds)
if run:
    assert max(nit.max(), nrunb.max()) < 65535, "this shape overflows the 16-bit fields of the DUO_PROF_RUN build"
    ctot = ctot * 0
npark, wmax = ((ctot.astype(np.int64) >> 16) & 0x7FF).astype(np.float64), int((ctot.astype(np.int64) >> 27).max())
assert npark.max() < 2047, "this shape parks too often for the 11-bit field of the DUO_PROF build"
ctot = (ctot.astype(np.int64) & 0xFFFF).astype(np.float64)
ev = ev.astype(np.int64); cyc = cyc.astype(np.int64)
ngen, nop = (ev & 0xFFFF).astype(np.float64), (ev >> 16).astype(np.float64)          # GENERAL bodies, generic op rounds
# (beside the generic op rounds' cycles, 5 bits that saturate: the flood op rounds that took the quiet body, 11 bits that saturate)
cgen, cop = (cyc & 0xFFFF).astype(np.float64) * 1024, ((cyc >> 16) & 31).astype(np.float64) * 1024
nquiet, cop_sat, nquiet_sat = (cyc >> 21).astype(np.float64), bool((((cyc >> 16) & 31) == 31).any()), bool(((cyc >> 21) == 2047).any())
ctot *= 4096
steady = os.environ.get("STEADY", "0") != "0"
if steady:   # (the word that held cgen | cop | nquiet: steady parks, 11 bits | steady leaves, 11 bits | their cycles / 4096, 10 bits, all saturating)
    nspark, nsleave, csx = (cyc & 0x7FF).astype(np.float64), ((cyc >> 11) & 0x7FF).astype(np.float64), (cyc >> 22).astype(np.float64) * 4096 + 2048
    steady_sat = int(((cyc & 0x7FF) == 2047).sum() + (((cyc >> 11) & 0x7FF) == 2047).sum()), int(((cyc >> 22) == 1023).sum())   # wavefronts with a saturated count, with saturated cycles
    print(f"steady fields: max steady parks {nspark.max():.0f}, max steady leaves {nsleave.max():.0f}, max cycles / 4096 {(cyc >> 22).max()}; saturated in {steady_sat[0]} (counts) and {steady_sat[1]} (cycles) of {len(cyc)} wavefronts")
    cgen, cop, nquiet = cgen * 0, cop * 0, nquiet * 0
# flood gossip rounds, flood op rounds, materialisations and their cycles (a build without flood mode leaves the generic numbers there: zero them)
flood = os.environ.get("FLOOD", "1") != "0"
nfg, nfop, nop2, nmat = [x.astype(np.float64) * flood for x in (up[:, 0], up[:, 1] & 0xFFFF, (up[:, 1] >> 16) & 0xFFF, (up[:, 1] >> 28) & 0xF)]
cfg_, cexit, cfop, cpk = [x.astype(np.float64) * 1024 * flood for x in (up[:, 2] & 0xFFFF, up[:, 2] >> 16, up[:, 3] & 0xFFFF, up[:, 3] >> 16)]
cpk += 512 * (npk > 0)   # (the fields are truncated to 1024 cycles; it matters for this small one alone)
if os.environ.get("MEMO", "0") != "0":
    lo1 = cyc   # reserved[1] of the lower instances; up[:, 2] is that of the upper ones
    nrep = ((lo1 & 0xFFFF) + (up[:, 2] & 0xFFFF)).astype(np.float64)
    nout = (((lo1 >> 16) & 0xFF) + ((up[:, 2] >> 16) & 0xFF)).astype(np.float64)
    nrec = (lo1 >> 24).astype(np.float64)
    ndrop = up[:, 3].astype(np.float64)   # reserved[2] of the upper instances: recordings dropped
    plan = run and os.environ.get("PLAN", "0") != "0"
    if plan:   # (PLAN=1: that word holds the block plans | the ops they took << 16 instead)
        nplan, nplanop = (up[:, 3] & 0xFFFF).astype(np.float64), (up[:, 3] >> 16).astype(np.float64)
        assert max(nplan.max(), nplanop.max()) < 65535, "this shape overflows the 16-bit fields of the DUO_PROF_PLAN build"
        ndrop = ndrop * 0
    assert ((lo1 >> 24) == (up[:, 2] >> 24)).all(), "the two instances of a wavefront carry the same count of recorded floods"
    out_sat = int((((lo1 >> 16) & 0xFF) == 255).sum() + (((up[:, 2] >> 16) & 0xFF) == 255).sum())
    print(f"latency {kw['latency']} ms {kw['latency_dist']}, {n} instances: sim kernel {sim_ms:.3f} ms (a -DDUO_PROF build: not the product's time)")
    print(f"per wavefront: wave-rounds {nwave.mean():.0f} (cluster rounds {rounds.mean():.0f} in the lower cluster), op wave-rounds {nop.mean() + nfop.mean():.0f} "
          f"({nfop.mean():.0f} flood op rounds, {nop.mean():.0f} generic, {nop2.mean():.0f} with two ops), full GENERAL bodies {ngen.mean():.0f}, "
          f"flood gossip rounds {nfg.mean():.0f}, parked gossip rounds {npk.mean():.0f}, parks {npark.mean():.0f} (longest wait {wmax}), reads executed ahead in read runs {nrun.mean():.0f}")
    print(f"flood memo, per wavefront (two clusters): floods recorded {nrec.mean():.1f} (max {nrec.max():.0f}), recordings dropped {ndrop.mean():.2f} (max {ndrop.max():.0f}), floods replayed {nrep.mean():.0f} (min {nrep.min():.0f}), "
          f"broadcasts taken outside the quiet body {nout.mean():.1f}" + (f" (the field is saturated in {out_sat} instances)" if out_sat else ""))
    if run:
        print(f"steady run, per wavefront (two clusters): iterations of the runs' loop {nit.mean():.0f}, broadcasts taken in runs {nrunb.mean():.0f} (counted among the floods replayed), "
              f"reads taken in runs {nrun.mean():.0f}; {(nrunb.mean() + nrun.mean()) / max(nit.mean(), 1):.2f} ops per iteration (the parks and the cycles are not carried by this build)")
        if plan:
            left = nrunb + nrun - nplanop
            print(f"block plan, per wavefront (two clusters): plans that took an op {nplan.mean():.0f}, the ops they took {nplanop.mean():.0f} ({nplanop.mean() / max(nplan.mean(), 1):.1f} per plan; min {nplanop.min():.0f}), "
                  f"ops the runs' loop still took {left.mean():.0f} (max {left.max():.0f}) (the recordings dropped are not carried by this build)")
    else:
        print(f"cycles per wavefront {ctot.mean():.3e} (max {ctot.max():.3e}): this build's, SGPR spills and all")
    sys.exit(0)
stretch = os.environ.get("STRETCH", "0") != "0"
if stretch:
    nst, nstr, ngg, cgg = (ev & 0xFFFF).astype(np.float64), (ev >> 16).astype(np.float64), (cyc & 0xFFFF).astype(np.float64), (cyc >> 16).astype(np.float64) * 1024
    assert max(nstr.max(), ngg.max(), (cyc >> 16).max()) < 65535, "this shape overflows the 16-bit fields of the DUO_PROF_STRETCH build"
    nin = nfg.mean() + npk.mean()   # flood gossip rounds, parked ones included: all of them run inside a stretch in a build with the stretch
    print(f"latency {kw['latency']} ms {kw['latency_dist']}, {n} instances: sim kernel {sim_ms:.3f} ms")
    print(f"per wavefront: wave-rounds {nwave.mean():.0f}, cycles {ctot.mean():.3e}; flood stretches {nst.mean():.0f}, rounds taken inside them {nstr.mean():.0f} "
          f"({nstr.mean() / max(nst.mean(), 1):.2f} per stretch; {100 * nstr.mean() / max(nin, 1):.1f} % of the {nin:.0f} flood gossip and parked rounds) at "
          f"{(cfg_.mean() + cpk.mean()) / max(nin, 1):.0f} cycles per round ({100 * (cfg_.mean() + cpk.mean()) / ctot.mean():.1f} % of the cycles)")
    print(f"generic gossip rounds, counted directly: {ngg.mean():.1f} per wavefront at {cgg.mean() / max(ngg.mean(), 1e-9):.0f} cycles each "
          f"({cgg.mean():.3e} cycles per wavefront, {100 * cgg.mean() / ctot.mean():.2f} %; the fields are truncated to 1024 cycles)")
    sys.exit(0)
nop_all = nop.mean() + nfop.mean()
print(f"latency {kw['latency']} ms {kw['latency_dist']}, {n} instances: sim kernel {sim_ms:.3f} ms")
nsched = ngen.mean() + nop_all
print(f"per wavefront: wave-rounds {nwave.mean():.0f} (cluster rounds {rounds.mean():.0f}), GENERAL {nsched:.0f} ({100 * nsched / nwave.mean():.1f} %): "
      f"op rounds {nop_all:.0f} ({100 * nop_all / max(nsched, 1):.1f} % of them), full GENERAL bodies {ngen.mean():.0f}")
if steady:
    print(f"cycles per wavefront {ctot.mean():.3e} (max {ctot.max():.3e})")
else:
    print(f"cycles per wavefront {ctot.mean():.3e} (max {ctot.max():.3e}); in GENERAL bodies {cgen.mean():.3e} ({100 * cgen.mean() / ctot.mean():.1f} %), "
          f"in generic op rounds {cop.mean():.3e} ({100 * cop.mean() / ctot.mean():.1f} %)")
ngos = nwave.mean() - nsched - nfg.mean() - npk.mean()          # generic gossip rounds: the loop's rest (a parked round in a generic body is counted as parked)
cgos = ctot.mean() - cgen.mean() - cop.mean() - cfop.mean() - cfg_.mean() - cpk.mean() - cexit.mean()   # (without flood mode: with the leaving rounds' R0, as ever; materialisations are part of the GENERAL bodies)
if not steady:
    print(f"cycles per GENERAL body {cgen.mean() / max(ngen.mean(), 1):.0f}, per generic op round ({nop.mean():.0f}) {cop.mean() / max(nop.mean(), 1):.0f}, "
          f"per generic gossip round ({ngos:.0f}) {cgos / max(ngos, 1):.0f}")
nfl = nfg.mean() + nfop.mean()
print(f"flood bodies {nfl:.0f} of {nwave.mean():.0f} wave-rounds ({100 * nfl / nwave.mean():.1f} %): flood gossip rounds {nfg.mean():.0f} at {cfg_.mean() / max(nfg.mean(), 1):.0f} cycles "
      f"({100 * cfg_.mean() / ctot.mean():.1f} % of the cycles), flood op rounds {nfop.mean():.0f} at {cfop.mean() / max(nfop.mean(), 1):.0f} ({100 * cfop.mean() / ctot.mean():.1f} %), "
      f"materialisations {nmat.mean():.1f} (counted to 15); R0 and exit test of the {nsched + npark.mean():.0f} rounds that leave the gossip loop or park a half "
      f"{cexit.mean() / max(nsched + npark.mean(), 1):.0f} each ({100 * cexit.mean() / ctot.mean():.1f} %)")
nopw = ngen.mean() + nop_all   # wave-rounds with an op (a GENERAL body of the main phase carries one as well)
print(f"wave-rounds with an op {nopw:.0f} per wavefront; reads executed ahead of such a round's op (read runs) {nrun.mean():.0f} per wavefront, "
      f"{nrun.mean() / max(nopw, 1):.2f} per wave-round with an op")
if steady:
    nleave = nsched + npark.mean()
    nfast = nspark.mean() + nsleave.mean()
    print(f"steady leave: steady parks {nspark.mean():.0f} of the {npark.mean():.0f} parks, steady leaves {nsleave.mean():.0f} of the {nop_all:.0f} op rounds per wavefront; of the {nleave:.0f} rounds "
          f"that leave the gossip loop or park a half {nfast:.0f} are fast ({100 * nfast / max(nleave, 1):.1f} %) at {csx.mean() / max(nfast, 1):.0f} cycles each from the stretch's exit "
          f"({100 * csx.mean() / ctot.mean():.1f} % of the cycles), {nleave - nfast:.0f} slow at {cexit.mean() / max(nleave - nfast, 1):.0f} each through R0 and the exit test ({100 * cexit.mean() / ctot.mean():.1f} %)")
if not stretch and not steady:
    print(f"quiet op rounds (every live half acts from flood mode: the body without the exchange) {nquiet.mean():.0f}{' or more' if nquiet_sat else ''} of the {nfop.mean():.0f} flood op rounds "
          f"per wavefront, {nfop.mean() - nquiet.mean():.0f} take the superset body" + ("; the generic op rounds' cycle field is saturated (31 x 1024 per wavefront)" if cop_sat else ""))
nop1 = nop_all - nop2.mean()
wmax_s = f"{wmax} or more" if wmax == 31 else str(wmax)   # (the field saturates)
print(f"paired op rounds: parks {npark.mean():.0f} per wavefront, parked gossip rounds {npk.mean():.0f} ({npk.mean() / max(npark.mean(), 1):.2f} per park, longest wait {wmax_s}) at "
      f"{cpk.mean() / max(npk.mean(), 1):.0f} cycles ({100 * cpk.mean() / ctot.mean():.1f} % of the cycles); op wave-rounds with one op {nop1:.0f}, with two {nop2.mean():.0f}")
