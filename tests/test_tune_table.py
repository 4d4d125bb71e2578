"""The tuning table shipped beside the library (mere-fusion_amd/tune/gfx950.txt), read the way the loader reads it (mf_conv_tune.hip, tune_cache()).

The loader reads `key bm bn wgm wgn nsplit ld` with `while (fscanf(...) == 7)`: one malformed line ends the read and every row after it is lost; a row its
validity check rejects is dropped with one line on stderr.  Either way the affected layers fall back to the cost model's pick and the output bits change from
box to box -- what the table exists to prevent.  So every row must parse, pass the loader's rules, be unique, belong to one network, and the table's
(network, precision, batch) points must be exactly the grid of mere-fusion_amd/tune_grid.py, which the parity tests sweep.  Each checker is also run on
mutated copies of the table to show that it fails on the fault it is there for."""
import os
import re

import pytest

from mere_fusion_amd.tune_grid import GRID

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TABLE = os.path.join(ROOT, "mere-fusion_amd", "tune", "gfx950.txt")

# tune_key() in mf_conv_tune.hip: the kernel generation, then 19 integers, then ':s' when the layer also leaves GroupNorm statistics
KEY_FIELDS = ("precision", "batch", "cin", "cout", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "transposed", "output_padding", "residual",
              "act", "in_h", "in_w", "upsample", "pad_hi", "in_c")
LINE_RE = re.compile(r"(g950k4((?::-?\d+){%d})(?::s)?) (-?\d+) (-?\d+) (-?\d+) (-?\d+) (-?\d+) (-?\d+)" % len(KEY_FIELDS))
PRECISION_NAMES = {0: "bf16", 1: "bf16x3"}                 # MF_PREC_BF16, MF_PREC_BF16X3 (include/merefusion.h)
PRECISION_IDS = {v: k for k, v in PRECISION_NAMES.items()}

# The loader's validity rules (mf_conv_tune.hip, `valid` in tune_cache() and mf_conv_tuned_valid).  KEEP IN SYNC with that lambda: a tile or operand path added there is added here.
TILES = {(64, 64, 2, 2), (128, 64, 2, 2), (128, 128, 2, 2), (256, 128, 4, 2), (256, 256, 2, 4), (128, 80, 4, 1)}   # (bm, bn, wgm, wgn)
LD_PATHS = {-1, 0, 2, 3, 4}

# Input map sizes (in_h, in_w) of the tunable layers of each network; the two sets are disjoint, so a key names its network.
WAV2LIP_MAPS = {(48, 48), (24, 24), (12, 12), (6, 6), (3, 3), (1, 1), (80, 16), (27, 16), (9, 6)}
MUSETALK_MAPS = {(s, s) for s in (256, 128, 64, 32, 16, 8, 4)} | {(1, 50)}


def read_table():
    with open(TABLE) as f:
        return f.read().splitlines()


def parse(lines):
    """-> (rows, problems); a row is (line number, key, {field: int}, (bm, bn, wgm, wgn, nsplit, ld))"""
    rows, problems = [], []
    for n, line in enumerate(lines, 1):
        m = LINE_RE.fullmatch(line)
        if not m:
            problems.append(f"line {n}: not `key bm bn wgm wgn nsplit ld`: {line!r}")
            continue
        fields = dict(zip(KEY_FIELDS, (int(v) for v in m.group(2)[1:].split(":"))))
        rows.append((n, m.group(1), fields, tuple(int(m.group(i)) for i in range(3, 9))))
    return rows, problems


def loader_rejects(cfg, precision=1, act=0):
    """The reason mf_conv_tune.hip's loader would drop this configuration of a key with this precision and activation, or None.  (KEEP IN SYNC with `valid` in
    tune_cache() and mf_conv_tuned_valid().)"""
    bm, bn, wgm, wgn, nsplit, ld = cfg
    if bm == 0:
        return None                                          # "the cost model's pick stays"
    if (ld == 3 or ld == 4) and wgm * wgn != 4:
        return f"ld {ld} needs a 4-wave tile"
    if bn == 80 and ld not in (3, 4):
        return "the 128 x 80 tile runs on the producer-wave kernels (ld 3 / 4) only"
    if (bm, bn, wgm, wgn) not in TILES:
        return f"tile {(bm, bn, wgm, wgn)} is not compiled"
    if not 1 <= nsplit <= 16:
        return f"split {nsplit} outside 1 .. 16"
    if ld not in LD_PATHS:
        return f"operand path ld {ld} does not exist"
    if (ld in (3, 4) or bn == 80) and precision != PRECISION_IDS["bf16x3"]:
        return "the producer-wave kernels (ld 3 / 4, the 128 x 80 tile) are bf16x3 only"
    if bn == 80 and act == 5:
        return "the 128 x 80 tile cannot pair GEGLU value / gate fragments"
    return None


def invalid_rows(rows):
    return [f"line {n}: {k}: {why}" for n, k, f, cfg in rows if (why := loader_rejects(cfg, f["precision"], f["act"]))]


def duplicate_keys(rows):
    first, problems = {}, []
    for n, k, _, _ in rows:
        if k in first:
            problems.append(f"line {n}: key of line {first[k]} again: {k}")
        else:
            first[k] = n
    return problems


def classify(rows):
    """-> (set of (network, precision name, batch), problems)"""
    points, problems = set(), []
    for n, k, f, _ in rows:
        hw = (f["in_h"], f["in_w"])
        nets = [net for net, maps in (("wav2lip", WAV2LIP_MAPS), ("musetalk", MUSETALK_MAPS)) if hw in maps]
        if len(nets) != 1:
            problems.append(f"line {n}: input map {hw} names {nets or 'no network'}: {k}")
        elif f["precision"] not in PRECISION_NAMES:
            problems.append(f"line {n}: precision {f['precision']} has no grid: {k}")
        else:
            points.add((nets[0], PRECISION_NAMES[f["precision"]], f["batch"]))
    return points, problems


def grid_points():
    return {(net, prec, b) for (net, prec), bs in GRID.items() for b in bs}


def grid_mismatch(points):
    want = grid_points()
    return [f"in the table, not in the grid: {p}" for p in sorted(points - want)] + \
           [f"in the grid, not in the table: {p}" for p in sorted(want - points)]


def all_problems(lines):
    rows, problems = parse(lines)
    points, cls = classify(rows)
    return problems + invalid_rows(rows) + duplicate_keys(rows) + cls + grid_mismatch(points)


@pytest.fixture(scope="module")
def lines():
    return read_table()


@pytest.fixture(scope="module")
def rows(lines):
    return parse(lines)[0]


def test_every_line_parses(lines):
    rows, problems = parse(lines)
    assert not problems, problems[:10]
    assert len(rows) == len(lines) > 0


def test_every_row_passes_the_loader_validity_rules(rows):
    assert not invalid_rows(rows), invalid_rows(rows)[:10]


def test_no_duplicate_keys(rows):
    assert not duplicate_keys(rows), duplicate_keys(rows)[:10]


def test_every_key_belongs_to_exactly_one_network(rows):
    assert not WAV2LIP_MAPS & MUSETALK_MAPS
    _, problems = classify(rows)
    assert not problems, problems[:10]


def test_table_matches_the_grid(rows):
    """The table holds every (network, precision, batch) of the grid and nothing else: the parity tests sweep exactly the configurations a deployment runs."""
    points, _ = classify(rows)
    assert not grid_mismatch(points), grid_mismatch(points)


def test_table_as_shipped_has_no_problems(lines):
    assert all_problems(lines) == []


def _replace_field(line, field, value):
    key, rest = line.split(" ", 1)
    parts = key.split(":")
    parts[1 + KEY_FIELDS.index(field)] = str(value)
    return ":".join(parts) + " " + rest


def _set_cfg(line, cfg):
    return line.split(" ", 1)[0] + " " + " ".join(str(v) for v in cfg)


def _first(lines, pred):
    return next(i for i, l in enumerate(lines) if pred(l))


def _mutate(lines, kind):
    out = list(lines)
    tuned = _first(out, lambda l: not l.endswith(" 0 0 0 0 0 -1"))
    mid = len(out) // 2
    if kind == "truncated_line":                      # a row cut short in the middle of the file (the loader stops reading there)
        out[mid] = out[mid].rsplit(" ", 1)[0]
    elif kind == "truncated_key":
        key, rest = out[mid].split(" ", 1)
        out[mid] = ":".join(key.split(":")[:10]) + " " + rest
    elif kind == "unknown_suffix":
        out[mid] = out[mid].replace(" ", ":x ", 1)
    elif kind == "invalid_tile":
        out[tuned] = _set_cfg(out[tuned], (96, 64, 2, 2, 1, 0))
    elif kind == "split_out_of_range":
        out[tuned] = _set_cfg(out[tuned], (64, 64, 2, 2, 17, 0))
    elif kind == "unknown_ld":
        out[tuned] = _set_cfg(out[tuned], (64, 64, 2, 2, 1, 1))
    elif kind == "producer_path_on_8_wave_tile":
        out[tuned] = _set_cfg(out[tuned], (256, 128, 4, 2, 1, 3))
    elif kind == "80_wide_tile_off_producer_path":
        out[tuned] = _set_cfg(out[tuned], (128, 80, 4, 1, 1, 2))
    elif kind == "producer_path_on_bf16_key":         # the bf16 library has no producer-wave kernel: the launch would fail
        i = _first(out, lambda l: l.split(":")[1] == "0" and not l.endswith(" 0 0 0 0 0 -1"))
        out[i] = _set_cfg(out[i], (128, 64, 2, 2, 1, 3))
    elif kind == "80_wide_tile_on_bf16_key":
        i = _first(out, lambda l: l.split(":")[1] == "0" and not l.endswith(" 0 0 0 0 0 -1"))
        out[i] = _set_cfg(out[i], (128, 80, 4, 1, 1, 4))
    elif kind == "80_wide_tile_on_geglu_key":
        i = _first(out, lambda l: l.split(":")[1] == "1" and l.split(" ")[0].split(":")[14] == "5")
        out[i] = _set_cfg(out[i], (128, 80, 4, 1, 1, 3))
    elif kind == "batch_outside_grid":
        out[mid] = _replace_field(out[mid], "batch", 7)
    elif kind == "grid_batch_missing":                # every row of Wav2Lip bf16 batch 128 gone
        drop = {n - 1 for n, _, f, _ in parse(out)[0] if f["batch"] == 128 and f["precision"] == 0}
        assert drop
        out = [l for i, l in enumerate(out) if i not in drop]
    elif kind == "duplicate_key":
        out.append(out[mid].split(" ", 1)[0] + " 0 0 0 0 0 -1")
    elif kind == "unknown_map_size":
        out[mid] = _replace_field(_replace_field(out[mid], "in_h", 96), "in_w", 96)
    else:
        raise AssertionError(kind)
    return out


MUTATIONS = {                                         # mutation -> the checker that must catch it
    "truncated_line": "parse", "truncated_key": "parse", "unknown_suffix": "parse",
    "invalid_tile": "valid", "split_out_of_range": "valid", "unknown_ld": "valid", "producer_path_on_8_wave_tile": "valid",
    "80_wide_tile_off_producer_path": "valid", "producer_path_on_bf16_key": "valid", "80_wide_tile_on_bf16_key": "valid",
    "80_wide_tile_on_geglu_key": "valid",
    "batch_outside_grid": "grid", "grid_batch_missing": "grid",
    "duplicate_key": "duplicates",
    "unknown_map_size": "classify",
}


@pytest.mark.parametrize("kind", sorted(MUTATIONS))
def test_checkers_fail_on_a_mutated_table(lines, kind):
    bad = _mutate(lines, kind)
    rows, parse_problems = parse(bad)
    points, cls = classify(rows)
    found = {"parse": parse_problems, "valid": invalid_rows(rows), "duplicates": duplicate_keys(rows), "classify": cls, "grid": grid_mismatch(points)}
    assert found[MUTATIONS[kind]], (kind, MUTATIONS[kind])
    assert all_problems(bad)
    # and only that checker: the mutation is the one fault in the copy
    assert [c for c, p in found.items() if p] == [MUTATIONS[kind]], {c: p[:2] for c, p in found.items() if p}


def test_loader_rules_accept_the_compiled_tiles():
    """The mirror of the loader's rules admits every compiled tile on an operand path it can run, and the cost model's pick: it is not rejecting everything."""
    for bm, bn, wgm, wgn in TILES:
        lds = (3, 4) if bn == 80 else (-1, 0, 2) + ((3, 4) if wgm * wgn == 4 else ())
        for ld in lds:
            for split in (1, 16):
                assert loader_rejects((bm, bn, wgm, wgn, split, ld)) is None, (bm, bn, wgm, wgn, split, ld)
                if bn != 80 and ld not in (3, 4):          # bf16 keys: everything but the producer-wave kernels
                    assert loader_rejects((bm, bn, wgm, wgn, split, ld), PRECISION_IDS["bf16"], 5) is None, (bm, bn, wgm, wgn, split, ld)
    assert loader_rejects((0, 0, 0, 0, 0, -1)) is None
