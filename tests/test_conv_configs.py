"""Every launch configuration of the convolution engine (mf_conv.hip, mf_conv_launch.hip, mf_conv_tune.hip, mf_conv_halo.hip, mf_conv_halo2.hip, mf_conv_thin.hip) against float64, at a derived
per-element bound, on the shapes where tiled kernels go wrong -- and proof, through mf_conv2d_launch_config, that each configuration actually ran.

Seam.  mf_conv2d_launch_config reports what a forward at a batch launches (family, tile, the split after every clamp, the operand path ld that runs, BK,
phases, GroupNorm statistics source), resolved by mf_conv_resolve -- the function the launch itself runs.  mf_conv2d_pin_config puts a (tile, split, ld)
into the slot the tuning table fills, with the table's rules and split clamp, so a pinned launch runs the production selection code.

Bound.  Inputs are exact in the storage format (conv_numerics.exact); each BatchNorm-folded weight is stored within U (hi + lo, or bf16 alone), a bf16x3
product drops lo_w lo_x (<= 2^-18 |w x|); the K products, the bias and the split-K partials are summed in fp32 (<= (K + 8) F32 of the magnitude
A = conv(|x|, |w'|) + |b'| (+ |x|, residual 1), first order), with K the largest per-phase tap count times cin; so before the activation
|e| <= (2 U + (K + 8) F32) A.  The activation multiplies that by its Lipschitz constant (ReLU 1, sigmoid 1/4, GELU / SiLU 1.13) and adds its own
evaluation error: sigmoid by __expf (the exponent's argument rounds: (4 + 0.4 A) F32), erff-GELU (8 F32 A), SiLU (t times sigmoid's: (8 + 0.4 A) F32 A).
A residual after the activation adds one fp32 rounding of |act| + |x|; the store rounds to U |y| (2 U |want|, as |y| may exceed |want|).
GEGLU y = v gelu(u): |gelu(u)| e_v + 1.13 |v| e_u + 1.13 e_v e_u, the erf approximation of its epilogue (erf_as, |error| <= 1.5e-7: 0.75e-7 |u v|) and
8 F32 of the product.  conv_numerics.conv_bound is this bound.

Outputs: the layer's output buffer is filled with NaN by a forward of an all-NaN input first (ReLU maps NaN to 0: a stale zero there still misses a
positive value), and the NCHW result tensor is pre-filled with NaN: an element no kernel wrote fails the comparison."""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conv_numerics import U, conv_bound, conv_ref, exact
import test_tune_table as TT

PRECS = ["bf16x3", "bf16"]
FAMILY = {0: "igemm", 1: "halo", 2: "halo_w", 3: "halo_w_split", 4: "twin", 5: "thin", 6: "f16q"}
STATS = {0: "none", 1: "epilogue", 2: "combine", 3: "pass"}

# ---- the configurations the selector can produce, per precision: (bm, bn, wgm, wgn, split, ld that runs) ----------------------------------------------
SPLITS = (1, 2, 3, 4, 6, 8, 12, 16)
TILES4 = [(64, 64, 2, 2), (128, 64, 2, 2), (128, 128, 2, 2)]
TILES8 = [(256, 128, 4, 2), (256, 256, 2, 4)]
TILE80 = (128, 80, 4, 1)
# (tile, ld pinned) -> the ld that runs: -1 resolves to 2 on the 4-wave tiles, to 0 on the 8-wave ones
PINS = {"bf16x3": [(t, ld) for t in TILES4 for ld in (-1, 0, 2, 3, 4)] + [(t, 0) for t in TILES8] + [(TILE80, 3), (TILE80, 4)],
        "bf16": [(t, ld) for t in TILES4 for ld in (-1, 0, 2)] + [(t, 0) for t in TILES8]}


def ld_runs(tile, ld):
    four = tile[2] * tile[3] == 4
    if ld in (3, 4):
        return ld
    return 2 if four and (2 if ld < 0 else ld) == 2 else 0


TARGETS = {prec: sorted({t + (s, ld_runs(t, ld)) for t, ld in pins for s in SPLITS}) for prec, pins in PINS.items()}


# ---- CPU: the reference, the target list ---------------------------------------------------------------------------------------------------------
REF_CASES = [  # (desc, bn) small random layers through torch.nn
    (dict(cin=5, cout=6, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=1, residual=0, in_h=7, in_w=6), True),
    (dict(cin=6, cout=6, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=3, residual=1, in_h=5, in_w=5), True),
    (dict(cin=4, cout=4, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, act=4, residual=2, in_h=4, in_w=3), False),
    (dict(cin=3, cout=5, kh=3, kw=3, stride_h=2, stride_w=2, pad_h=0, pad_w=0, act=2, residual=0, in_h=9, in_w=8, pad_hi=1), True),
    (dict(cin=4, cout=3, kh=3, kw=3, stride_h=2, stride_w=2, pad_h=1, pad_w=1, act=0, residual=0, in_h=4, in_w=5, transposed=1, output_padding=1), True),
    (dict(cin=3, cout=4, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=4, residual=0, in_h=3, in_w=4, upsample=1), False),
    (dict(cin=5, cout=8, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, act=5, residual=0, in_h=4, in_w=4), False),
]


@pytest.mark.parametrize("i", range(len(REF_CASES)))
def test_conv_ref_is_torch_nn(i):
    """conv_ref against torch.nn modules: Conv2d / ConvTranspose2d, then BatchNorm2d.eval(), F.pad, nearest upsampling, the activation functions"""
    d, bn = REF_CASES[i]
    g = torch.Generator().manual_seed(i)
    x = torch.randn(2, d["cin"], d["in_h"], d["in_w"], generator=g, dtype=torch.float64)
    if d.get("transposed"):
        m = nn.ConvTranspose2d(d["cin"], d["cout"], d["kh"], stride=d["stride_h"], padding=d["pad_h"], output_padding=d["output_padding"]).double()
    else:
        m = nn.Conv2d(d["cin"], d["cout"], d["kh"], stride=d["stride_h"], padding=d["pad_h"]).double()
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64))
        m.bias.copy_(torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
    bnp = None
    seq = [m]
    if bn:
        b2 = nn.BatchNorm2d(d["cout"]).double().eval()
        with torch.no_grad():
            b2.weight.uniform_(0.5, 2, generator=g); b2.bias.normal_(generator=g)
            b2.running_mean.normal_(generator=g); b2.running_var.uniform_(0.5, 2, generator=g)
        seq.append(b2)
        bnp = (b2.weight.detach(), b2.bias.detach(), b2.running_mean, b2.running_var)
    with torch.no_grad():
        xin = F.interpolate(x, scale_factor=2.0, mode="nearest") if d.get("upsample") else x
        xin = F.pad(xin, (0, d["pad_hi"], 0, d["pad_hi"])) if d.get("pad_hi") else xin
        pre = nn.Sequential(*seq)(xin)
        if d["residual"] == 1:
            pre = pre + x
        a = d["act"]
        if a == 5:
            h = d["cout"] // 2
            want = pre[:, :h] * F.gelu(pre[:, h:])
        else:
            want = [lambda t: t, torch.relu, torch.sigmoid, F.gelu, F.silu][a](pre)
        if d["residual"] == 2:
            want = want + x
        got, mag = conv_ref(x, m.weight.detach(), m.bias.detach(), d, bnp)
    assert got.shape == want.shape
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.all(mag["pre"] >= pre.abs() - 1e-12)              # the magnitude dominates the pre-activation it bounds


def _kt_min(f):
    """smallest per-phase count of 64-deep K tiles of a table key's layer (mf_conv_plan_create): taps x cin_pad / 8 groups of 8 channels, 8 groups a tile"""
    cpg = (f["cin"] + 7) // 8
    if f["upsample"]:
        taps = [4]
    elif f["transposed"]:
        s, k, p = f["stride_h"], f["kh"], f["pad_h"]
        taps = [1] if s == 1 else [sum((r + p - ky) % s == 0 for ky in range(k)) * sum((c + p - kx) % s == 0 for kx in range(k))
                                       for r in range(s) for c in range(s)]
    else:
        taps = [f["kh"] * f["kw"]]
    return min((t * cpg + 7) // 8 for t in taps)


def test_every_table_configuration_is_a_target():
    """every (tile, split, ld) of the shipped tuning table is in the target list -- as written, or as the launch clamps it for every layer that uses it --
    so a table regenerated with a configuration the sweep never ran fails here, on the CPU"""
    rows, problems = TT.parse(TT.read_table())
    assert not problems
    prec_name = {0: "bf16", 1: "bf16x3"}
    missing, seen = [], set()
    for n, key, f, cfg in rows:
        bm, bn, wgm, wgn, s, ld = cfg
        if bm == 0:
            continue
        prec = prec_name[f["precision"]]
        tile = (bm, bn, wgm, wgn)
        seen.add((prec,) + tile + (s, ld))
        runs = tile + (s, ld_runs(tile, ld))
        clamped = tile + (1 if f["cout"] % 4 else max(1, min(s, _kt_min(f))), ld_runs(tile, ld))
        if runs not in TARGETS[prec] and clamped not in TARGETS[prec]:
            missing.append(f"line {n}: {key}: {cfg}")
    assert not missing, missing[:10]
    assert len(seen) >= 50                                 # (the table holds 76 distinct configurations; the check is not vacuous)


def test_every_pinnable_target_passes_the_loader_rules():
    for prec, pins in PINS.items():
        p = TT.PRECISION_IDS[prec]
        for t, ld in pins:
            for s in SPLITS:
                assert TT.loader_rejects(t + (s, ld), p, 0) is None, (prec, t, s, ld)
    # and what the sweep expects to be refused is refused by the mirror too
    assert TT.loader_rejects(TILE80 + (1, 3), TT.PRECISION_IDS["bf16"], 0)
    assert TT.loader_rejects((64, 64, 2, 2, 1, 4), TT.PRECISION_IDS["bf16"], 0)
    assert TT.loader_rejects(TILE80 + (1, 3), TT.PRECISION_IDS["bf16x3"], 5)


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------------------------
def _desc(d):
    from mere_fusion_amd import _lib
    f = dict(transposed=0, output_padding=0, residual=0, upsample=0, pad_hi=0)
    f.update(d)
    return _lib.MfConv2dDesc(**{k: f[k] for k in ("cin", "cout", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w", "transposed", "output_padding",
                                                   "residual", "act", "in_h", "in_w", "upsample", "pad_hi")}), f


class Layer:
    """one mf_conv2d handle with seeded parameters, its float64 reference and the checks"""

    def __init__(self, d, prec, seed, bn=False):
        from mere_fusion_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        _lib.init_device(0)
        self.cd, self.d = _desc(d)
        self.prec = prec
        rng = np.random.default_rng(seed)
        self.rng = rng
        ci, co, kh, kw = self.d["cin"], self.d["cout"], self.d["kh"], self.d["kw"]
        shape = (ci, co, kh, kw) if self.d["transposed"] else (co, ci, kh, kw)
        self.w = (rng.standard_normal(shape) / math.sqrt(ci * kh * kw)).astype(np.float32)
        self.b = (0.5 * rng.standard_normal(co)).astype(np.float32)
        self.bn = tuple(a.astype(np.float32) for a in (rng.uniform(0.5, 2, co), 0.5 * rng.standard_normal(co), 0.5 * rng.standard_normal(co),
                                                        rng.uniform(0.5, 2, co))) if bn else None
        ptr = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None
        self.h = C.c_void_p()
        self.rc = self.lib.mf_conv2d_create(C.byref(self.cd), ptr(self.w), ptr(self.b), *((ptr(a) for a in self.bn) if bn else (None,) * 4),
                                            _lib.PRECISIONS[prec], C.byref(self.h))
        self.err = self.lib.mf_last_error().decode() if self.rc else ""
        if not self.rc:
            oh, ow = C.c_int(), C.c_int()
            self.lib.mf_conv2d_out_shape(self.h, C.byref(oh), C.byref(ow))
            self.oh, self.ow = oh.value, ow.value

    def close(self):
        if self.h:
            self.lib.mf_conv2d_destroy(self.h)
            self.h = C.c_void_p()

    def pin(self, batch, tile, split, ld):
        rc = self.lib.mf_conv2d_pin_config(self.h, batch, *tile, split, ld)
        return rc, (self.lib.mf_last_error().decode() if rc else "")

    def config(self, batch, groups=0):
        info = (C.c_int * 11)()
        self.L.check(self.lib.mf_conv2d_launch_config(self.h, batch, groups, info, 11))
        v = list(info)
        return dict(family=FAMILY[v[0]], tile=tuple(v[1:5]), split=v[5], ld=v[6], bk=v[7], nphase=v[8], stats=STATS[v[9]], pinned=v[10])

    def input(self, batch):
        return torch.from_numpy(exact(self.rng, (batch, self.d["cin"], self.d["in_h"], self.d["in_w"]), self.prec)).cuda()

    def forward(self, x, groups=0):
        B = x.shape[0]
        co = self.d["cout"] // 2 if self.d["act"] == 5 else self.d["cout"]
        nan_in = torch.full_like(x, float("nan"))
        y = torch.full((B, co, self.oh, self.ow), float("nan"), device="cuda")
        self.L.check(self.lib.mf_conv2d_forward(self.h, C.c_void_p(nan_in.data_ptr()), C.c_void_p(y.data_ptr()), B, None))
        y.fill_(float("nan"))
        st = None
        if groups:
            st = torch.full((B, groups, 2), 7.0, dtype=torch.float64, device="cuda")
            self.L.check(self.lib.mf_conv2d_forward_stats(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), groups, C.c_void_p(st.data_ptr()), B, None))
        else:
            self.L.check(self.lib.mf_conv2d_forward(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), B, None))
        torch.cuda.synchronize()
        return y, st

    def check(self, x, y, what):
        """y against the float64 reference at the derived bound; returns the worst error in units of U A"""
        want, mag = conv_ref(x, torch.from_numpy(self.w), torch.from_numpy(self.b), self.d,
                             tuple(torch.from_numpy(a) for a in self.bn) if self.bn else None)
        bound = conv_bound(want, mag, self.d, self.prec, self.d["cin"])
        got = y.double()
        err = (got - want).abs()
        ok = err <= bound                                   # NaN (an element nobody wrote) fails
        if not bool(ok.all()):
            bad = (~ok).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} elements over the bound; first at {bad}: got {got[tuple(bad)].item():.6e} "
                                 f"want {want[tuple(bad)].item():.6e} bound {bound[tuple(bad)].item():.3e}")
        A = mag["mv"] * (mag["mu"] + 1) if self.d["act"] == 5 else mag["pre"] + mag["res"]
        return float((err / (U[self.prec] * A + 1e-300)).max())


WORST = {}     # (family, precision) -> worst error seen, in units of U A (printed: the record of the measured margins)


def _note(family, prec, e):
    k = (family, prec)
    WORST[k] = max(WORST.get(k, 0.0), e)
    print(f"[worst] {family} {prec} {e:.4f} U A")


# ---- the pinned sweep ----------------------------------------------------------------------------------------------------------------------------
# Layer shapes built to hit the edges: A: cin k^2 = 1044 (not a multiple of 64; 17 K tiles: every split up to 16 launches, none divides K), M = 198 and
# N = 116 (multiples of no tile, N of 4); B: 6 K tiles (split 3 leaves 2 K steps per split, fewer than any producer-wave ring has stages), M = 182, N = 40
# (below every channel tile); C: N = 70 (N % 4 != 0: the launch must take split 1 whatever is pinned), stride 2.
SHAPE_A = dict(cin=116, cout=116, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, in_h=9, in_w=11)
SHAPE_B = dict(cin=40, cout=40, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, in_h=7, in_w=13)
SHAPE_C = dict(cin=72, cout=70, kh=3, kw=3, stride_h=2, stride_w=2, pad_h=1, pad_w=1, in_h=12, in_w=10)
# epilogue flavours (act, residual, BatchNorm), rotated over the cases; every one must meet the one-pass store and the split-K combine
FLAVOURS = [(a, r, bn) for a in range(5) for r in (0, 1, 2) for bn in (0, 1)]
BATCH = 2


def _one(prec, shape, tile, split, ld, flav, hits, seen_flav, label):
    act, res, bn = flav
    if shape is SHAPE_C:
        res = 0                                              # (cin != cout)
    lay = Layer(dict(shape, act=act, residual=res), prec, seed=hash((tile, split, ld, act, res, bn)) % 2 ** 31, bn=bool(bn))
    try:
        assert not lay.rc, lay.err
        rc, msg = lay.pin(BATCH, tile, split, ld)
        assert rc == 0, (label, msg)
        cfg = lay.config(BATCH)
        assert cfg["family"] == "igemm" and cfg["pinned"] == 1 and cfg["tile"] == tile, (label, cfg)
        assert cfg["ld"] == ld_runs(tile, ld), (label, cfg)
        if shape["cout"] % 4:
            assert cfg["split"] == 1, (label, cfg)          # the split-K quads would straddle pixels
        elif shape is SHAPE_A:
            assert cfg["split"] == split, (label, cfg)      # 17 K tiles: nothing clamps
        else:
            assert cfg["split"] == min(split, 6), (label, cfg)
        x = lay.input(BATCH)
        y, _ = lay.forward(x)
        e = lay.check(x, y, f"{label} {cfg}")
        _note("igemm", prec, e)
        hits.add(cfg["tile"] + (cfg["split"], cfg["ld"]))
        seen_flav.add((act, res, bn, cfg["split"] > 1))
    finally:
        lay.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_pinned_configurations_vs_fp64(lib_built, prec):
    """every (tile, split, ld) the tuning table may name for this precision, pinned onto edge shapes, against float64 at the derived bound; the coverage
    gate at the end: the report showed every target on a case that ran and passed, and every epilogue flavour met both the one-pass store and the combine"""
    t0 = time.time()
    hits, seen_flav = set(), set()
    i = 0
    for tile, ld in PINS[prec]:
        for split in SPLITS:
            for shape in (SHAPE_A, SHAPE_B, SHAPE_C) if split <= 3 else (SHAPE_A,):
                _one(prec, shape, tile, split, ld, FLAVOURS[i % len(FLAVOURS)], hits, seen_flav, f"{prec} {tile} split {split} ld {ld}")
                i += 1
    # flavours that missed a path (the rotation is coarse): once more each, on 64 x 64 with split 1 / split 4
    for act, res, bn in FLAVOURS:
        for split in (1, 4):
            if (act, res, bn, split > 1) not in seen_flav:
                _one(prec, SHAPE_A, TILES4[0], split, 0, (act, res, bn), hits, seen_flav, f"{prec} flavour {(act, res, bn)} split {split}")
    missing = sorted(set(TARGETS[prec]) - hits)
    assert not missing, f"targets never reported by a case that passed: {missing}"
    assert all((a, r, b, s) in seen_flav for a, r, b in FLAVOURS for s in (False, True))
    print(f"[pinned {prec}] {i} cases, {len(hits)} configurations, worst {WORST.get(('igemm', prec), 0):.3f} U A, {time.time() - t0:.1f} s")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
def test_pin_refusals(lib_built, prec):
    """configurations no compiled kernel of the precision runs, and layers the table does not serve, are refused with a message -- never launched"""
    lay = Layer(dict(SHAPE_A, cout=128, act=5), prec, seed=1)
    try:
        assert not lay.rc, lay.err
        bad = [((96, 64, 2, 2), 1, 0), ((64, 64, 2, 2), 17, 0), ((64, 64, 2, 2), 1, 1), ((256, 128, 4, 2), 1, 3), (TILE80, 1, 2),
               (TILE80, 1, 3)]                           # the last: GEGLU on the 80-channel tile (five fragments per wave do not pair value / gate)
        if prec == "bf16":
            bad += [((64, 64, 2, 2), 1, 3), ((128, 128, 2, 2), 2, 4)]
        for tile, s, ld in bad:
            rc, msg = lay.pin(BATCH, tile, s, ld)
            assert rc != 0 and msg, (tile, s, ld)
        assert lay.config(BATCH)["pinned"] == 0
        rc, _ = lay.pin(BATCH, (64, 64, 2, 2), 2, 0)
        assert rc == 0 and lay.config(BATCH)["pinned"] == 1
        rc, _ = lay.pin(BATCH, (0, 0, 0, 0), 0, -1)
        assert rc == 0 and lay.config(BATCH)["pinned"] == 0
    finally:
        lay.close()
    for d in (dict(cin=40, cout=28, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, in_h=9, in_w=9, act=0),          # narrow tile
              dict(cin=40, cout=64, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, in_h=20, in_w=20, act=1)):       # halo kernel
        lay = Layer(d, prec, seed=2)
        try:
            rc, msg = lay.pin(BATCH, (64, 64, 2, 2), 1, 0)
            assert rc != 0 and "table does not serve" in msg, msg
        finally:
            lay.close()
    # descriptors the seam cannot serve are refused at creation, with the reason
    for d in (dict(cin=8, cout=48, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=1, pad_w=1, in_h=8, in_w=8, act=5),          # GEGLU cout % 32
              dict(cin=8, cout=8, kh=3, kw=3, stride_h=1, stride_w=1, pad_h=0, pad_w=0, in_h=2, in_w=2, act=0, transposed=1),   # convT s1 on 2 x 2
              dict(cin=8, cout=8, kh=1, kw=1, stride_h=1, stride_w=1, pad_h=0, pad_w=0, in_h=8, in_w=8, act=0, upsample=1)):     # upsample + 1x1
        lay = Layer(d, prec, seed=3)
        assert lay.rc != 0 and lay.err, d
        lay.close()


# ---- paths chosen by shape -----------------------------------------------------------------------------------------------------------------------
def _c(cin, cout, k, s, p, h, w, **kw):
    sh, sw = (s, s) if isinstance(s, int) else s
    return dict(cin=cin, cout=cout, kh=k, kw=k, stride_h=sh, stride_w=sw, pad_h=p, pad_w=p, in_h=h, in_w=w, **kw)


# (name, desc, batch, family, tile (bm / ph, bn) or None, split: 1, ">1" or None)
SHAPE_PATHS = [
    ("128x16 split", _c(24, 12, 3, 1, 1, 12, 12, act=1), 2, "igemm", (128, 16), ">1"),
    ("128x16 one-pass", _c(8, 12, 1, 1, 0, 12, 12, act=2), 2, "igemm", (128, 16), 1),
    ("128x32 split", _c(24, 28, 3, 1, 1, 12, 12, act=3, residual=0), 2, "igemm", (128, 32), ">1"),
    ("128x32 one-pass", _c(8, 28, 1, 1, 0, 12, 12, act=4), 2, "igemm", (128, 32), 1),
    ("16x64 split", _c(64, 72, 3, 1, 1, 4, 4, act=4), 1, "igemm", (16, 64), ">1"),
    ("16x64 one-pass", _c(8, 72, 1, 1, 0, 4, 4, act=0), 1, "igemm", (16, 64), 1),
    ("16x64 residual after act", _c(72, 72, 1, 1, 0, 4, 4, act=3, residual=2), 1, "igemm", (16, 64), ">1"),
    ("geglu cout 32 split", _c(40, 32, 3, 1, 1, 6, 6, act=5), 2, "igemm", (128, 32), ">1"),
    ("geglu cout 32 one-pass", _c(8, 32, 1, 1, 0, 6, 6, act=5), 2, "igemm", (128, 32), 1),
    ("geglu cout 64 split", _c(72, 64, 3, 1, 1, 7, 9, act=5), 2, "igemm", None, None),
    ("geglu cout 96 one-pass", _c(8, 96, 1, 1, 0, 40, 40, act=5), 2, "igemm", None, None),
    ("convT s2 k3 p1 op1", _c(40, 36, 3, 2, 1, 6, 6, act=1, transposed=1, output_padding=1), 2, "igemm", None, None),
    ("convT s1 1x1", _c(64, 48, 3, 1, 0, 1, 1, act=0, transposed=1), 2, "igemm", None, None),
    ("upsample", _c(24, 40, 3, 1, 1, 8, 7, act=1, upsample=1), 2, "igemm", None, None),
    ("stride 2", _c(20, 44, 3, 2, 1, 11, 9, act=2), 2, "igemm", None, None),
    ("stride (3,1)", _c(32, 64, 3, (3, 1), 1, 20, 8, act=1), 2, "igemm", None, None),
    ("stride (3,2)", _c(48, 68, 3, (3, 2), 1, 9, 6, act=4), 2, "igemm", None, None),
    ("pad_hi", _c(36, 40, 3, 2, 0, 11, 13, act=0, pad_hi=1), 2, "igemm", None, None),
    ("halo 8x64", _c(40, 68, 3, 1, 1, 64, 64, act=1), 4, "halo", (8, 64), None),
    ("halo 4x64", _c(72, 68, 3, 1, 1, 64, 64, act=0, residual=0), 2, "halo", (4, 64), None),
    ("halo 4x32 wide", _c(68, 68, 3, 1, 1, 32, 32, act=2, residual=1), 1, "halo", (4, 32), None),
    ("halo 8x32", _c(40, 28, 3, 1, 1, 128, 128, act=1), 2, "halo", (8, 32), None),
    ("halo 4x32 narrow", _c(20, 28, 3, 1, 1, 20, 20, act=0), 1, "halo", (4, 32), None),
    ("halo_w 16x128 4x2", _c(32, 128, 3, 1, 1, 96, 96, act=1), 8, "halo_w", (16, 128), None),
    ("halo_w 16x256", _c(40, 256, 3, 1, 1, 96, 96, act=0), 8, "halo_w", (16, 256), None),
    ("halo_w split", _c(512, 256, 3, 1, 1, 32, 32, act=1), 16, "halo_w_split", (16, 256), ">1"),
    ("halo_w split, residual is the input", _c(512, 512, 3, 1, 1, 32, 32, act=1, residual=1), 8, "halo_w_split", (16, 256), ">1"),
    ("twin", _c(512, 256, 3, 1, 1, 32, 32, act=2), 2, "twin", None, None),
    ("thin k7 s1", _c(6, 16, 7, 1, 3, 32, 32, act=1), 2, "thin", None, None),
    ("thin k3 s1", _c(12, 28, 3, 1, 1, 24, 24, act=2), 2, "thin", None, None),
    ("thin k3 s2 cin 3", _c(3, 20, 3, 2, 1, 48, 40, act=0), 2, "thin", None, None),
    ("thin k3 s2 cin 16", _c(16, 32, 3, 2, 1, 40, 40, act=1), 2, "thin", None, None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", SHAPE_PATHS, ids=[c[0] for c in SHAPE_PATHS])
def test_shape_chosen_paths_vs_fp64(lib_built, prec, case):
    name, d, B, fam, tile, split = case
    if prec == "bf16" and fam == "halo_w" and B > 4:
        B = 4                                                 # (the bf16 run keeps its own tile choice at a smaller batch; the family is what is checked)
    lay = Layer(d, prec, seed=sum(map(ord, name)), bn=d["act"] != 5 and not d.get("transposed") and d["cin"] % 3 == 0)
    try:
        assert not lay.rc, lay.err
        cfg = lay.config(B)
        if not (prec == "bf16" and B != case[2]):
            assert cfg["family"] == fam, (name, cfg)
            if tile:
                assert cfg["tile"][:2] == tile, (name, cfg)
        if split == 1:
            assert cfg["split"] == 1, (name, cfg)
        elif split == ">1":
            assert cfg["split"] > 1, (name, cfg)
        x = lay.input(B)
        y, _ = lay.forward(x)
        _note(cfg["family"], prec, lay.check(x, y, f"{name} {prec} {cfg}"))
    finally:
        lay.close()


# ---- GroupNorm statistics ------------------------------------------------------------------------------------------------------------------------
# (name, desc, batch, groups, pin (tile, split, ld) or None, the source the report must name)
STATS_CASES = [
    ("epilogue", _c(40, 40, 3, 1, 1, 8, 8, act=0), 2, 4, ((64, 64, 2, 2), 1, 0), "epilogue"),          # 10 channels per group
    ("epilogue cpg 8", _c(40, 64, 3, 1, 1, 8, 8, act=1), 2, 8, ((64, 64, 2, 2), 1, 2), "epilogue"),
    ("combine", _c(40, 40, 3, 1, 1, 8, 8, act=0), 2, 4, ((64, 64, 2, 2), 3, 0), "combine"),
    ("combine residual after act", _c(40, 40, 3, 1, 1, 7, 9, act=4, residual=2), 2, 8, ((128, 64, 2, 2), 2, 2), "combine"),
    ("pass: 8-wave tile", _c(40, 40, 3, 1, 1, 8, 8, act=0), 2, 4, ((256, 128, 4, 2), 1, 0), "pass"),
    ("pass: tile across samples", _c(40, 40, 3, 1, 1, 7, 9, act=1), 2, 4, ((64, 64, 2, 2), 1, 0), "pass"),
    ("pass: halo", _c(40, 64, 3, 1, 1, 32, 32, act=1), 2, 16, None, "pass"),
    ("halo split combine", _c(512, 256, 3, 1, 1, 32, 32, act=0), 16, 32, None, "combine"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", STATS_CASES, ids=[c[0] for c in STATS_CASES])
def test_groupnorm_statistics_sources(lib_built, prec, case):
    """mf_conv2d_forward_stats from each source the report names, against float64 statistics of the stored y (gate of test_conv_wide.py: 2e-6 of the
    largest moment); y itself within the bound and bit-identical to the plain forward's"""
    name, d, B, groups, pin, source = case
    lay = Layer(d, prec, seed=sum(map(ord, name)))
    try:
        assert not lay.rc, lay.err
        if pin:
            rc, msg = lay.pin(B, *pin)
            assert rc == 0, msg
        cfg = lay.config(B, groups)
        assert cfg["stats"] == source, (name, cfg)
        x = lay.input(B)
        y, st = lay.forward(x, groups)
        _note(cfg["family"], prec, lay.check(x, y, f"{name} {prec} {cfg}"))
        yg = y.double().reshape(B, groups, -1)
        want = torch.stack([yg.sum(-1), (yg * yg).sum(-1)], dim=-1)
        scale = want.abs().amax(dim=(0, 1)) + 1e-30
        err = float(((st - want).abs() / scale).max())
        assert err <= 2e-6, (name, cfg, err)
        y2, _ = lay.forward(x)
        assert torch.equal(y, y2)
    finally:
        lay.close()


# ---- batch behaviour -----------------------------------------------------------------------------------------------------------------------------
BATCH_CASES = [
    ("igemm split", _c(116, 116, 3, 1, 1, 9, 11, act=3, residual=2), ((64, 64, 2, 2), 16, 0)),
    ("igemm producer waves", _c(116, 116, 3, 1, 1, 9, 11, act=4), ((128, 64, 2, 2), 3, 3)),
    ("igemm cost model", _c(40, 44, 3, 2, 1, 13, 11, act=1), None),
    ("halo", _c(40, 68, 3, 1, 1, 24, 24, act=1), None),
    ("halo_w / twin", _c(512, 256, 3, 1, 1, 32, 32, act=0), None),
    ("thin", _c(12, 28, 3, 1, 1, 24, 24, act=2), None),
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("case", BATCH_CASES, ids=[c[0] for c in BATCH_CASES])
def test_batch_growth_and_identical_items(lib_built, prec, case):
    """one handle at batch 1, then 4, then 2 (the split-K workspace grows, then a smaller launch reuses it), each against float64; then 4 identical
    items, whose outputs must agree bit for bit at every position"""
    name, d, pin = case
    lay = Layer(d, prec, seed=sum(map(ord, name)))
    try:
        assert not lay.rc, lay.err
        if pin and pin[2] >= 3 and prec == "bf16":
            pin = (pin[0], pin[1], 0)
        for B in (1, 4, 2):
            if pin:
                assert lay.pin(B, *pin)[0] == 0
            cfg = lay.config(B)
            x = lay.input(B)
            y, _ = lay.forward(x)
            _note(cfg["family"], prec, lay.check(x, y, f"{name} {prec} batch {B} {cfg}"))
        x = lay.input(1).repeat(4, 1, 1, 1)
        if pin:
            assert lay.pin(4, *pin)[0] == 0
        y, _ = lay.forward(x)
        for k in range(1, 4):
            assert torch.equal(y[k], y[0]), (name, k)
    finally:
        lay.close()
