"""msim_journal_svg_rows (csrc/journal_svg.cpp; the contract: the last section of include/maelsim_journal.h): one journal as the
Lamport diagram of the reference's net/viz.clj.  The output is parsed with xml.etree and held to a restatement of the geometry in
Python doubles: the window, the columns, one group per delivered pair with its translation, angle, length and fill, the labels'
cadence, the endpoints' lines, the height, the notice of a truncated journal.  Needs no device."""
import ctypes as C
import math
import re
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from maelstrom_amd import _abi as A
from maelstrom_amd import engine as E

import journal_cases as K
from test_journal_messages import oracle_journals

SVG, XLINK = "{http://www.w3.org/2000/svg}", "{http://www.w3.org/1999/xlink}"
INIT = (A.MSG_TYPES.index("init"), A.MSG_TYPES.index("init_ok"))
TOL = 1e-3


def restated(cfg, events, names):
    """-> (columns in order, {name: x}, steps, truncated, the pairs [(x0, y0, angle, length, fill, type)] in journal order of the recv)"""
    n, slots = cfg.n_nodes, max(cfg.concurrency, cfg.n_nodes)
    bound = 10000 + 4 * n + 1
    win = [i for i in range(min(len(events), bound)) if int(events["msg"][i]) & 0x7F not in INIT]
    truncated = len(win) > 10000
    win = win[:10000]
    eps = sorted({int(events["route"][i]) >> s & 0xFF for i in win for s in (0, 8)})
    def key(e):
        m = re.fullmatch(r"([a-z])(\d+)", names(e))
        return (0, m.group(1), int(m.group(2))) if m else (1, names(e), 0)
    cols = [names(e) for e in sorted(eps, key=key)]
    x = {c: (k + 0.5) / len(cols) * 1200 for k, c in enumerate(cols)}
    y = lambda step: 20 * (1.5 + step)
    froms, pairs = {}, []
    for k, i in enumerate(win):
        msg, route, step = int(events["msg"][i]), int(events["route"][i]), k + 1
        src, dest = route & 0xFF, route >> 8 & 0xFF
        if not msg & 0x80:
            froms[msg >> 8] = (names(src), step)
            continue
        if msg >> 8 not in froms:
            continue
        (fn, fs) = froms[msg >> 8]
        x0, y0, x1, y1 = x[fn], y(fs), x[names(dest)], y(step)
        fill = "#FF1E90" if A.MSG_TYPES[msg & 0x7F] == "error" else "#81BFFC" if "c" in (names(src)[0], names(dest)[0]) else "#000"
        pairs.append((x0, y0, math.atan2(y1 - y0, x1 - x0) / 2 / math.pi * 360, math.hypot(x1 - x0, y1 - y0), fill, A.MSG_TYPES[msg & 0x7F],
                      f"{names(src)} → {names(dest)} {A.MSG_TYPES[msg & 0x7F]}"))
    return cols, x, len(win), truncated, pairs


def namer(cfg, service="lin-kv"):
    n, slots = cfg.n_nodes, max(cfg.concurrency, cfg.n_nodes)
    return lambda e: f"n{e}" if e < n else f"c{e - n}" if e < n + slots else service


def groups(root):
    return {g.get("class"): g for g in root.findall(SVG + "g")}


def held_to_the_restatement(cfg, events, names):
    root = ET.fromstring(E.journal_svg(cfg, events))
    cols, x, steps, truncated, pairs = restated(cfg, events, names)
    assert root.tag == SVG + "svg" and float(root.get("width")) == 1200 and abs(float(root.get("height")) - 20 * (7 + steps)) < TOL
    g = groups(root)
    # one group per delivered pair of the window
    drawn = g["messages"].findall(SVG + "g")
    assert len(drawn) == len(pairs)
    for d, (x0, y0, angle, length, fill, typ, title) in zip(drawn, pairs):
        tx, ty, rot = (float(v) for v in re.fullmatch(r"translate\((\S+) (\S+)\) rotate\((\S+)\)", d.get("transform")).groups())
        assert abs(tx - x0) < TOL and abs(ty - y0) < TOL and abs(rot - angle) < TOL, (d.get("transform"), x0, y0, angle)
        rect, use, glow, label = list(d)
        assert rect.tag == SVG + "rect" and abs(float(rect.get("width")) - (length - 4)) < TOL and rect.get("fill") == fill
        assert (float(rect.get("x")), float(rect.get("y")), float(rect.get("height"))) == (0, -2.5, 5) and rect.find(SVG + "title").text == title
        assert use.get(XLINK + "href") == "#ahead" and abs(float(use.get("x")) - length) < TOL
        assert glow.get("filter") == "url(#glow)" and label.get("filter") is None and glow.text == label.text == typ
        assert abs(float(label.get("x")) - length / 2) < TOL and float(label.get("y")) == -4
        left = not -90 < angle < 90
        assert (label.get("transform") is not None) == left == (glow.get("transform") is not None)
        if left:
            assert abs(float(re.fullmatch(r"rotate\(180 (\S+) 0\)", label.get("transform")).group(1)) - length / 2) < TOL
    # the endpoints: a line each, a name each every 50 steps
    lines = g["node-lines"].findall(SVG + "line")
    assert [round(float(l.get("x1")), 3) for l in lines] == [round(x[c], 3) for c in cols]
    assert all(l.get("stroke") == "#ccc" and abs(float(l.get("y1")) - 30) < TOL and abs(float(l.get("y2")) - 20 * (2.5 + steps)) < TOL for l in lines)
    labels = g["node-labels"].findall(SVG + "text")
    want = [(c, s) for c in cols for s in range(0, steps, 50)]
    assert [(t.text, round(float(t.get("y")), 3), t.get("fill")) for t in labels] == [(c, 20 * (1.0 + s), "#000" if s == 0 else "#aaa") for c, s in want]
    assert all(abs(float(t.get("x")) - x[t.text]) < TOL for t in labels)
    assert ("truncated" in g) == truncated
    assert {d.get("id") for d in root.find(SVG + "defs")} == {"ahead", "glow"}
    return root, cols, steps, pairs


@pytest.mark.parametrize("name", ["ack-retry", "echo", "lin-kv proxy", "broadcast"])
def test_oracle_journals_drawn(lib, name):
    cfg, ora = oracle_journals(name)
    ev = ora.events(0)
    root, cols, steps, pairs = held_to_the_restatement(cfg, ev, namer(cfg))
    init = np.isin(ev["msg"] & 0x7F, INIT)
    assert init.any() and steps == int((~init).sum())   # the init traffic is absent
    assert len(pairs) == int(((ev["msg"] & 0x80 != 0) & ~init).sum()) > 50
    assert not any(t.text in ("init", "init_ok") for t in root.iter(SVG + "text"))
    assert {p[4] for p in pairs} >= {"#81BFFC"} and any(not -90 < p[2] < 90 for p in pairs)
    if name == "lin-kv proxy":
        assert cols[-1] == "lin-kv" and cols[0] == "c0" and "n0" in cols   # the service's column is the last
        assert "#FF1E90" in {p[4] for p in pairs} and "#000" in {p[4] for p in pairs}   # error replies; node <-> service traffic


def test_a_truncated_journal(lib):
    """10050 events that are no init traffic: 10000 are drawn and the notice stands below them; one fewer than the limit + 1: no notice"""
    cfg = E.test_config("broadcast", node_count=3, rate=10, time_limit=5, seed=1)
    bc = A.MSG_TYPES.index("broadcast")
    ev = K.journal([K.ev(i, i // 2, i % 2 == 1, i // 2 % 3, (i // 2 + 1) % 3, kind=bc) for i in range(10050)])
    root, cols, steps, pairs = held_to_the_restatement(cfg, ev, namer(cfg))
    assert steps == 10000 and len(pairs) == 5000 and cols == ["n0", "n1", "n2"]
    note = groups(root)["truncated"]
    line, text = note.find(SVG + "line"), note.find(SVG + "text")
    assert (float(line.get("x1")), float(line.get("x2")), line.get("stroke")) == (30, 1170, "#D96918") and abs(float(line.get("y1")) - 20 * (1.5 + 10002)) < TOL
    assert text.text == "Additional network events not shown" and abs(float(text.get("y")) - 20 * (1.5 + 10003)) < TOL and text.get("fill") == "#D96918"
    root, cols, steps, pairs = held_to_the_restatement(cfg, ev[:10000], namer(cfg))
    assert steps == 10000 and "truncated" not in groups(root)
    # a journal far longer than the window: what lies behind position 10000 + 4 n + 1 is not looked at
    long = np.concatenate([ev, ev, ev])
    assert E.journal_svg(cfg, long) == E.journal_svg(cfg, long[:10013])


def test_calling_convention(lib):
    cfg, ora = oracle_journals("echo")
    ev = np.ascontiguousarray(ora.events(0))
    L, need = A.load(), C.c_size_t()
    assert L.msim_journal_svg_rows(C.byref(cfg), ev.ctypes.data, len(ev), None, 0, C.byref(need)) == 0 and need.value > 1000
    small = C.create_string_buffer(16)
    assert L.msim_journal_svg_rows(C.byref(cfg), ev.ctypes.data, len(ev), small, 16, None) == A.E_RANGE
    assert L.msim_journal_svg_rows(None, ev.ctypes.data, len(ev), None, 0, C.byref(need)) == A.E_INVALID
    assert L.msim_journal_svg_rows(C.byref(cfg), None, 1, None, 0, C.byref(need)) == A.E_INVALID
    assert L.msim_journal_svg_rows(C.byref(cfg), ev.ctypes.data, len(ev), None, 16, None) == A.E_INVALID
    bad = ev.copy()
    bad["msg"][3] = (bad["msg"][3] & ~np.uint32(0x7F)) | np.uint32(0x7E)   # no such message type
    assert L.msim_journal_svg_rows(C.byref(cfg), bad.ctypes.data, len(bad), None, 0, C.byref(need)) == A.E_RANGE
    empty = ET.fromstring(E.journal_svg(cfg, ev[:0]))
    assert float(empty.get("height")) == 140 and not groups(empty)["messages"].findall(SVG + "g")
