"""The Wav2Lip and VAE edge kernels of csrc/mf_aux.hip one at a time: k_faces_u8 and k_faces_u8_rows (uint8 crops -> 8-channel planes), k_vae_image_u8,
k_head<32> (1 x 1 conv + sigmoid, both output layouts) and the fp32 <-> plane converters k_nchw_to_act / k_act_to_nchw.

The uint8 producers are compared bit for bit with the NumPy model of tests/aux_kernels_ref.py through mf_faces_u8_forward / mf_vae_image_u8_forward
(csrc/mf_nn_api.hip), which hand back the whole poisoned buffer -- batch + 1 items and the allocation's tail -- as fp32 (hi + lo).  That sum is exact, so
bit equality of it pins the pair; the bf16 run of the same case returns the hi plane alone, and sum - hi (exact again) is the lo plane, compared on its own.
The head is compared with float64 through mf_head_sigmoid_forward under a gate derived in test_head_nchw_hwc_and_bytes; the converters run behind
Net.set_input / Net.output.  The host tests at the top pin the model to hand-derived bit patterns.
"""
import ctypes as C

import numpy as np
import pytest

import aux_kernels_ref as R

PRECS = ["bf16x3", "bf16"]
SHAPES = [(1, 2, 2), (3, 5, 7), (2, 6, 4), (5, 9, 13)]           # (batch, H, W): odd H with H != W; 585 pixels = 2 workgroups + a partial one


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pair(code, value):
    """(hi, lo) bit patterns of one code's value"""
    hi, lo = R.split(np.float32([value(np.uint8(code))]), "bf16x3")
    return int(R.bf16_bits(hi)[0]), int(R.bf16_bits(lo)[0])


# ---- host: the model against known answers ---------------------------------------------------------------------------------------------------------------
def test_model_known_answers_of_the_faces_value():
    # 1 / 255 = 2^-8 * 256 / 255 = 2^-8 * (1 + 2^-8 + 2^-16 + 2^-24 + ...): fraction bits 8 and 16 are set, the rest (2^-24 + 2^-32 + ...) is just above
    # half of the last place 2^-23, so bit 23 rounds up: fraction field 0x8000 | 0x80 | 0x1, exponent -8 -> 127 - 8 = 0x77 -> 0x3B800000 | 0x008081
    assert _bits(R.faces_value(np.uint8([1])))[0] == 0x3B808081
    # hi: the dropped half 0x8081 is above 0x8000, so 0x3B80 rounds up to 0x3B81 = 2^-8 (1 + 2^-7).
    # lo: v - hi = 2^-8 (2^-8 + 2^-16 + 2^-23 - 2^-7) = -2^-17 (2 - 2^-7 - 2^-14) = -2^-17 * 1.1111110_1111111b; seven fraction bits stay and the dropped
    # 1111111b is above half, so it rounds up to -2^-17 * 1.1111111b: sign 1, exponent 127 - 17 = 0x6E, fraction 0x7F -> 1|0110 1110|111 1111 = 0xB77F
    assert _pair(1, R.faces_value) == (0x3B81, 0xB77F)
    # 128 / 255 = 2^-1 * 256 / 255: the same significand at exponent -1 (0x7E): 0x3F008081 -> hi 0x3F01; lo's exponent moves by 7 too: 127 - 10 = 0x75 ->
    # 1|0111 0101|111 1111 = 0xBAFF
    assert _bits(R.faces_value(np.uint8([128])))[0] == 0x3F008081
    assert _pair(128, R.faces_value) == (0x3F01, 0xBAFF)
    assert _pair(255, R.faces_value) == (0x3F80, 0x0000)          # 255 / 255 = 1.0 exactly, nothing left for lo
    assert _pair(0, R.faces_value) == (0x0000, 0x0000)


def test_model_known_answers_of_the_vae_value():
    assert _pair(255, R.vae_value) == (0x3F80, 0x0000) and R.vae_value(np.uint8([255]))[0] == 1.0       # (1 - 0.5) / 0.5
    assert _pair(0, R.vae_value) == (0xBF80, 0x0000) and R.vae_value(np.uint8([0]))[0] == -1.0          # (0 - 0.5) / 0.5
    # the double quotient rounds to the same fp32 as the faces' fp32 quotient here (the double keeps bits 8 .. 48 and drops less than half a place)
    assert _bits(R.vae_unit(np.uint8([1, 128]))).tolist() == [0x3B808081, 0x3F008081]
    # code 128: f - 0.5 = 2^-1 (2^-8 + 2^-16 + 2^-23) exactly, / 0.5 exactly: 2^-8 (1 + 2^-8 + 2^-15): fraction field 0x8000 | 0x100 -> 0x3B808100;
    # hi rounds up to 0x3B81 (0x8100 > 0x8000); lo = 2^-8 (2^-8 + 2^-15 - 2^-7) = -2^-16 (1 - 2^-7) = -2^-17 (2 - 2^-6) = -2^-17 * 1.111111b exactly:
    # 1|0110 1110|111 1110 = 0xB77E
    assert _bits(R.vae_value(np.uint8([128])))[0] == 0x3B808100
    assert _pair(128, R.vae_value) == (0x3B81, 0xB77E)


def test_model_split_reproduces_every_code():
    codes = np.arange(256, dtype=np.uint8)
    for value in (R.faces_value, R.vae_value):
        v = value(codes)
        hi, lo = R.split(v, "bf16x3")
        back = hi.astype(np.float64) + lo.astype(np.float64)
        assert np.all(np.abs(back - v.astype(np.float64)) <= 2.0 ** -17 * np.abs(v.astype(np.float64)))
        assert np.array_equal(_bits(hi + lo), _bits(back.astype(np.float32)))                          # the fp32 sum a read-back forms is exact
        assert R.split(v, "bf16")[1] is None and np.array_equal(_bits(R.split(v, "bf16")[0]), _bits(hi))
    assert np.all(np.diff(R.faces_value(codes)) > 0) and np.all(np.diff(R.vae_value(codes)) > 0)


def test_model_channels_mask_and_placement():
    faces = (np.arange(3 * 5 * 7 * 3) % 256).astype(np.uint8).reshape(3, 5, 7, 3) | 1                           # no zero code: a masked value is told from a kept one
    v = R.faces_channels(faces)
    assert R.keep_rows(5).tolist() == [True, True, False, False, False] and R.keep_rows(2).tolist() == [True, False]
    assert np.all(v[:, :2, :, :3] == R.faces_value(faces[:, :2])) and np.all(v[:, 2:, :, :3] == 0) and np.all(v[..., 3:6] == R.faces_value(faces))
    assert np.all(v[..., 6:] == 0)
    img = faces
    u = R.vae_channels(img, 1)
    assert np.all(u[:, 2:, :, :3] == -1.0) and np.all(u[:, :2, :, 0] == R.vae_value(img[:, :2, :, 2])) and np.all(u[..., 3:] == 0)
    assert np.array_equal(R.vae_channels(img, 0)[:, :, :, 2], R.vae_value(img[..., 0]))                 # B of BGR lands in channel 2
    want, written = R.padded(v, 1, "bf16x3")
    full = want[:-R.TAIL].reshape(4, 7, 9, 8)
    assert written.sum() == v.size and np.array_equal(_bits(full[:3, 1:6, 1:8]), _bits(sum(R.split(v, "bf16x3"))))
    assert np.all(want[~written] == np.float32(-1231.375)) and np.all(R.padded(v, 1, "bf16")[0][~written] == np.float32(-1232.0))
    assert np.all(full[3] == np.float32(-1231.375)) and np.all(full[:, 0] == np.float32(-1231.375)) and np.all(full[:, :, 8] == np.float32(-1231.375))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------------
def _u8_calls(batch, H, W, seed):
    """uint8 [calls, batch, H, W, 3]: every code 0 .. 255 at least once over the calls (one call where the shape holds 256 bytes), the rest seeded draws"""
    per = batch * H * W * 3
    calls = -(-256 // per)
    rng = np.random.default_rng(seed)
    data = np.concatenate([np.arange(256), rng.integers(0, 256, calls * per - 256)]).astype(np.uint8)
    rng.shuffle(data)
    assert len(np.unique(data)) == 256
    return data.reshape(calls, batch, H, W, 3)


HEAD_GEOMS = [(32, 0, 3, 5, 7), (48, 8, 3, 5, 7), (32, 0, 2, 9, 13)]          # (cbuf, coff, batch, H, W)
HEAD_FORCED = [30.0, -30.0, 120.0, -120.0]


def _head_case(batch, H, W, seed):
    """x [batch, H * W, 32], w [3, 32], b [3] (fp32) and the flat pixel indices of the four forced pixels.  Every pixel is t * u + noise along one unit
    direction u, and filter k is alpha_k * u + noise, so the logits are about alpha_k * t, t uniform in [-12, 12], while the magnitude sum the FMA chain
    rounds against stays near |z| + 4 instead of growing with cancellation: the derived gate stays small enough that few products sit within it of an
    integer.  The forced pixels are t * u exactly, t = +-30 and +-120 (channel 0; the other two filters scale them by -0.8 and 0.6)."""
    rng = np.random.default_rng(seed)
    T = H * W
    u = rng.standard_normal(32)
    u /= np.linalg.norm(u)
    alpha = np.float64([1.0, -0.8, 0.6])
    w = (alpha[:, None] * u[None] + 0.05 * rng.standard_normal((3, 32))).astype(np.float32)
    b = np.float32([0.3, -0.2, 0.1])
    t = rng.uniform(-12, 12, (batch, T, 1))
    x = (t * u + 0.3 * rng.standard_normal((batch, T, 32))).astype(np.float32)
    forced = [0, T - 1, (batch // 2) * T + T // 2, batch * T - 1]
    for p, target in zip(forced, HEAD_FORCED):
        x.reshape(-1, 32)[p] = (target * u).astype(np.float32)
    return x, w, b, forced


def _head_reference(x, w, b, prec):
    """float64 (s, z) over the stored inputs and the gate: the derivation of aux_kernels_ref.head_gate_terms itself (see test_head_nchw_hwc_and_bytes)"""
    xs = sum(p for p in R.split(x, prec) if p is not None)
    s, z, A = R.head64(xs, w, b)
    logit, ev = R.head_gate_terms(z, A)
    derived = float(logit.max() + ev)
    return s, z, derived, derived


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("geom", HEAD_GEOMS, ids=lambda g: "cbuf%d_coff%d_%dx%dx%d" % g)
def test_head_inputs_keep_the_byte_exceptions_under_one_percent(prec, geom):
    cbuf, coff, batch, H, W = geom
    x, w, b, forced = _head_case(batch, H, W, cbuf + H)
    s, z, derived, gate = _head_reference(x, w, b, prec)
    p = (s * 255.0).transpose(0, 2, 1).reshape(-1, 3)                              # [pixel, k]
    near = np.abs(p - np.rint(p)) <= 255 * gate
    seeded = np.ones(len(p), bool)
    seeded[forced] = False
    print(f"[head inputs {geom} {prec}] derived {derived:.3e} gate {gate:.3e} logits [{z.min():.1f}, {z.max():.1f}] seeded values near an integer: "
          f"{near[seeded].mean():.4f}")
    # The four forced pixels sit on 0 or 255 by construction (all three filters saturate there: 12 of the 315 values of the smaller shape), so the
    # 1 % is counted over the seeded pixels; the GPU test excludes nothing but values inside 255 * gate of an integer, forced or not.
    assert near[seeded].mean() < 0.01 and near[forced].all()
    z0 = z[:, 0].reshape(-1)
    assert all(abs(z0[p] - tgt) < 0.2 * abs(tgt) for p, tgt in zip(forced, HEAD_FORCED))         # (the filter's noise moves alpha_0 by 0.05 N(0, 1))
    rest = np.delete(z0, forced)
    assert rest.min() < -10 and rest.max() > 10 and np.abs(rest).max() < 16        # the ordinary logits span about [-12, 12]
    assert gate < 1e-5                                                            # (2 * 255 * gate stays well under the 1 % the exceptions may take)


# ---- GPU plumbing ----------------------------------------------------------------------------------------------------------------------------------------
def _L():
    from mere_fusion_amd import _lib
    _lib.init_device(0)
    return _lib, _lib.lib()


def _full_len(batch, H, W, halo):
    return (batch + 1) * (H + 2 * halo) * (W + 2 * halo) * 8 + R.TAIL


def _rows_arg(rows):
    return None if rows is None else (C.c_int * len(rows))(*[int(r) for r in rows])


def run_faces(faces, rows, halo, prec, batch=None):
    """mf_faces_u8_forward -> the flat fp32 image of the whole buffer (batch + 1 items and the tail).  faces: uint8 [n, H, W, 3], the batch itself or the pool"""
    import torch
    _lib, L = _L()
    n, H, W, _ = faces.shape
    batch = (n if rows is None else len(rows)) if batch is None else batch
    fd = torch.from_numpy(np.ascontiguousarray(faces)).cuda()
    full = torch.empty(_full_len(batch, H, W, halo), device="cuda")
    _lib.check(L.mf_faces_u8_forward(fd.data_ptr(), _rows_arg(rows), n if rows is not None else 0, H, W, halo, batch, _lib.PRECISIONS[prec], full.data_ptr(), None),
               "faces_u8_forward")
    return full.cpu().numpy()


def run_vae_image(img, halo, half_mask, prec):
    import torch
    _lib, L = _L()
    batch, H, W, _ = img.shape
    d = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    full = torch.empty(_full_len(batch, H, W, halo), device="cuda")
    _lib.check(L.mf_vae_image_u8_forward(d.data_ptr(), H, W, halo, half_mask, batch, _lib.PRECISIONS[prec], full.data_ptr(), None), "vae_image_u8_forward")
    return full.cpu().numpy()


def run_head(x, w, b, g, hwc255, prec):
    """mf_head_sigmoid_forward -> fp32 [batch, 3, H, W] (hwc255 0) or [batch, H, W, 3] (hwc255 1)"""
    import torch
    _lib, L = _L()
    batch = x.shape[0]
    xd, wd, bd = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda()
    out = torch.full((batch, g.h, g.w, 3) if hwc255 else (batch, 3, g.h, g.w), float("nan"), device="cuda")
    _lib.check(L.mf_head_sigmoid_forward(xd.data_ptr(), C.byref(g), wd.data_ptr(), bd.data_ptr(), hwc255, out.data_ptr(), batch, _lib.PRECISIONS[prec], None),
               "head_sigmoid_forward")
    return out.cpu().numpy()


def assert_planes(got, got_hi, v, halo, prec, what):
    """the whole buffer against the model: poison outside the interior of the first B items (ring, item B, tail), the interior bit for bit.  got_hi: the bf16
    run of the same case (bf16x3 only): the lo plane is got - got_hi"""
    want, written = R.padded(v, halo, prec)
    assert got.shape == want.shape
    poison = np.float32(-1231.375 if prec == "bf16x3" else -1232.0)
    bad = _bits(got)[~written] != _bits(poison)
    assert not bad.any(), f"{what}: {int(bad.sum())} elements outside the interior were written (first at flat index {np.flatnonzero(~written)[np.argmax(bad)]})"
    bad = _bits(got)[written] != _bits(want)[written]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {int(written.sum())} interior values differ from the model (first at interior index {int(np.argmax(bad))})"
    if prec == "bf16x3":
        hi, lo = R.split(v, prec)
        assert np.array_equal(_bits(got_hi[written]), _bits(hi).ravel()), f"{what}: hi plane"
        assert np.array_equal(_bits(got[written] - got_hi[written]), _bits(lo).ravel()), f"{what}: lo plane"


def _interior(got, batch, H, W, halo):
    return got[:-R.TAIL].reshape(batch + 1, H + 2 * halo, W + 2 * halo, 8)[:batch, halo:halo + H, halo:halo + W]


# ---- faces -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_faces_u8_bit_equal_to_the_model(lib_built, prec, halo, shape):
    batch, H, W = shape
    for call, faces in enumerate(_u8_calls(batch, H, W, H * 100 + W)):
        got = run_faces(faces, None, halo, prec)
        got_hi = run_faces(faces, None, halo, "bf16") if prec == "bf16x3" else None
        v = R.faces_channels(faces)
        assert_planes(got, got_hi, v, halo, prec, f"faces {shape} halo {halo} call {call}")
        inner = _interior(got, batch, H, W, halo)
        assert np.all(_bits(inner[..., 6:]) == 0)                                                   # exact +0.0 in both planes
        assert np.all(inner[:, H // 2:, :, :3] == 0) and np.array_equal(_bits(inner[:, :H // 2, :, :3]), _bits(inner[:, :H // 2, :, 3:6]))
        if prec == "bf16":
            assert np.array_equal(_bits(inner[..., 3:6]), _bits(R.bf16_rne(R.faces_value(faces))))  # no lo plane: hi alone is still the exact rounding


POOL_ROWS = {"one": [6], "repeats": [3, 3, 0, 6, 3], "256": 256, "257": 257, "513": 513}


def _pool_and_rows(name):
    rng = np.random.default_rng(len(name) * 7 + 1)
    pool = rng.integers(0, 256, (7, 4, 6, 3)).astype(np.uint8)
    rows = POOL_ROWS[name]
    if isinstance(rows, int):                                # more than one launch: every pool face on both sides of every 256-row boundary
        rows = rng.integers(0, 7, rows).tolist()
        for at in range(255, len(rows), 256):
            rows[at - 1:at + 2] = [(at + j) % 7 for j in range(len(rows[at - 1:at + 2]))]
    return pool, rows


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("name", list(POOL_ROWS))
def test_pooled_faces_equal_the_direct_kernel_on_the_gathered_faces(lib_built, prec, halo, name):
    pool, rows = _pool_and_rows(name)
    batch = len(rows)
    got = run_faces(pool, rows, halo, prec)
    direct = run_faces(pool[rows], None, halo, prec)
    assert np.array_equal(_bits(got), _bits(direct))                                               # every item, ring, the item behind the batch, tail
    got_hi = run_faces(pool, rows, halo, "bf16") if prec == "bf16x3" else None
    assert_planes(got, got_hi, R.faces_channels(pool[rows]), halo, prec, f"pooled faces {name} halo {halo}")
    last = got[:-R.TAIL].reshape(batch + 1, -1)[batch]
    assert np.all(_bits(last) == _bits(np.float32(-1231.375 if prec == "bf16x3" else -1232.0)))     # the item behind `batch` is untouched


@pytest.mark.gpu
def test_pooled_faces_refuse_a_row_outside_the_pool(lib_built):
    import torch
    _lib, L = _L()
    pool = torch.from_numpy(_pool_and_rows("one")[0]).cuda()
    for rows, bad_at in (([-1], 0), ([7], 0), ([0, 6, 7, 1], 2), ([2] * 300 + [-1], 300)):
        full = torch.full((_full_len(len(rows), 4, 6, 1),), 7.25, device="cuda")
        rc = L.mf_faces_u8_forward(pool.data_ptr(), _rows_arg(rows), 7, 4, 6, 1, len(rows), _lib.PRECISIONS["bf16x3"], full.data_ptr(), None)
        msg = L.mf_last_error().decode()
        assert rc == -1 and f"rows[{bad_at}] = {rows[bad_at]}" in msg and "pool of 7" in msg, (rows[bad_at], msg)
        torch.cuda.synchronize()
        assert bool((full == 7.25).all())                                                          # refused before anything was launched
    got = run_faces(pool.cpu().numpy(), [0, 6], 1, "bf16x3")                                        # (and the legal ends of the range still run)
    assert not np.any(_interior(got, 2, 4, 6, 1)[..., 3:6] == np.float32(-1231.375))


# ---- VAE image -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("half_mask", [0, 1])
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_vae_image_u8_bit_equal_to_the_model(lib_built, prec, half_mask, halo, shape):
    batch, H, W = shape
    for call, img in enumerate(_u8_calls(batch, H, W, H * 100 + W + 50)):
        got = run_vae_image(img, halo, half_mask, prec)
        got_hi = run_vae_image(img, halo, half_mask, "bf16") if prec == "bf16x3" else None
        assert_planes(got, got_hi, R.vae_channels(img, half_mask), halo, prec, f"vae image {shape} halo {halo} mask {half_mask} call {call}")
        inner = _interior(got, batch, H, W, halo)
        assert np.all(_bits(inner[..., 3:]) == 0)
        if half_mask:
            assert np.all(inner[:, H // 2:, :, :3] == -1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("half_mask", [0, 1])
def test_vae_image_channel_order_and_mask_rows(lib_built, prec, half_mask):
    rng = np.random.default_rng(5)
    batch, H, W = 3, 5, 7
    img = np.stack([rng.integers(0, 80, (batch, H, W)), rng.integers(90, 170, (batch, H, W)), rng.integers(180, 256, (batch, H, W))], -1).astype(np.uint8)   # B, G, R
    got = run_vae_image(img, 1, half_mask, prec)
    inner = _interior(got, batch, H, W, 1)
    kept = inner[:, :H // 2] if half_mask else inner
    lim = R.vae_value(np.uint8([80, 90, 170, 180])).astype(np.float64) + np.float64([1, -1, 1, -1]) * 2.0 ** -8           # (a bf16 hi plane moves a value by < 2^-8)
    assert np.all(kept[..., 0] > lim[3]) and np.all((kept[..., 1] > lim[1]) & (kept[..., 1] < lim[2])) and np.all(kept[..., 2] < lim[0])   # R, G, B
    src = img[:, :H // 2] if half_mask else img
    for c in range(3):
        want = sum(p for p in R.split(R.vae_value(src[..., 2 - c]), prec) if p is not None)
        assert np.array_equal(_bits(kept[..., c]), _bits(want))
    if half_mask:
        assert np.all(inner[:, 2:, :, :3] == -1.0) and not np.any(inner[:, :2, :, :3] == -1.0)     # H = 5: rows 0-1 kept, rows 2-4 masked


# ---- head ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("halo", [0, 1])
@pytest.mark.parametrize("geom", HEAD_GEOMS, ids=lambda g: "cbuf%d_coff%d_%dx%dx%d" % g)
def test_head_nchw_hwc_and_bytes(lib_built, prec, halo, geom):
    """The gate.  k_head forms each logit z with 32 chained fp32 FMAs starting from the bias; every FMA rounds a partial sum no larger than
    A = |b| + sum |w_c x_c|, so |dz| <= 32 u A with u = 2^-24.  The sigmoid's slope s (1 - s) is at most 1/4 (and at most e^-|z|, which is what keeps
    the +-30 and +-120 pixels, whose A is large, out of the maximum), so the logit contributes min(1/4, e^-|z|) * 32 u A to s.  Evaluating
    1 / (1 + expf(-z)) adds expf's 1 ulp (2 u relative), the rounding of the sum (u) and a division within 2.5 ulp (5 u), relative to s <= 1, and the
    product with 255 of the other layout one more u: 9 u = 5.4e-7.  derived = max over the case's elements of the first term + 9 u, evaluated in
    float64 on the inputs (1.62e-6 to 1.68e-6 over the cases, printed); the gate is that bound itself, 1 x (the allowance is 4 x).  expf overflows to inf
    at -z > 88.7 and flushes to 0 at -z < -103: the -+120 pixels give exactly 0 and 1, off the float64 value by e^-120.
    Measured on an MI355X: L-inf 8.0e-8 to 1.01e-7 over the 12 cases, a sixteenth of the gate."""
    from mere_fusion_amd import _lib
    cbuf, coff, batch, H, W = geom
    x, w, b, forced = _head_case(batch, H, W, cbuf + H)
    s64, z, derived, gate = _head_reference(x, w, b, prec)
    s64 = s64.reshape(batch, 3, H, W)
    g = _lib.MfRowsGeom(cbuf, coff, 32, H, W, halo)
    nchw = run_head(x, w, b, g, 0, prec)
    hwc = run_head(x, w, b, g, 1, prec)
    err = np.abs(nchw.astype(np.float64) - s64)
    print(f"[head {geom} halo {halo} {prec}] L-inf {err.max():.3e} derived {derived:.3e} gate {gate:.3e}")
    assert np.all(np.isfinite(nchw)) and nchw.min() >= 0 and nchw.max() <= 1
    assert err.max() <= gate
    flat = nchw[:, 0].reshape(-1)
    assert abs(flat[forced[2]] - 1) <= gate and abs(flat[forced[3]]) <= gate and abs(flat[forced[0]] - 1) <= gate and abs(flat[forced[1]]) <= gate
    # one kernel, one s: the other layout is the same fp32 value times 255 at the transposed position
    assert np.array_equal(_bits(hwc), _bits(nchw.transpose(0, 2, 3, 1) * np.float32(255)))
    # the bytes the paste kernel truncates them to
    p64 = s64.transpose(0, 2, 3, 1) * 255.0
    assert hwc.min() >= 0 and hwc.max() <= 255
    diff = hwc.astype(np.uint8).astype(np.int64) - np.floor(p64).astype(np.int64)
    near = np.abs(p64 - np.rint(p64)) <= 255 * gate
    assert np.abs(diff).max() <= 1 and not np.any((diff != 0) & ~near), (int(np.abs(diff).max()), int(((diff != 0) & ~near).sum()))


# ---- the fp32 <-> plane converters behind Net.set_input / Net.output ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("Cn", [3, 13])
def test_converters_round_trip_pad_channels_and_views(lib_built, prec, Cn):
    import torch
    from mere_fusion_amd.avatar.net import Net
    batch, H, W = 2, 5, 7
    rng = np.random.default_rng(Cn)
    x = (rng.standard_normal((batch, Cn, H, W)) * 10.0 ** rng.integers(-3, 4, (batch, Cn, 1, 1))).astype(np.float32)
    x.reshape(-1)[:6] = np.float32([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 0.0, 1e-30, -3e38])      # bf16 ties both ways, zero, tiny, huge
    n = Net(batch, prec, "cuda")
    buf = n.buffer(Cn, H, W, 1)
    Cb = (Cn + 7) // 8 * 8
    n.set_input(buf, torch.full((batch, Cb, H, W), 7.0))                                        # the pad channels hold something before the call under test
    n.set_input(buf, torch.from_numpy(x))
    got = n.output(buf, Cb, batch).cpu().numpy()
    hi, lo = R.split(x, prec)
    want = hi if lo is None else hi + lo
    assert np.array_equal(_bits(got[:, :Cn]), _bits(want))
    assert np.all(_bits(got[:, Cn:]) == 0)
    x64 = x.astype(np.float64)
    if prec == "bf16x3":
        assert np.all(np.abs(got[:, :Cn].astype(np.float64) - x64) <= 2.0 ** -16 * np.abs(x64))
    else:
        assert np.array_equal(_bits(got[:, :Cn]), _bits(R.bf16_rne(x)))
    if Cn == 13:
        view = n.output(buf, 5, batch, coff=8).cpu().numpy()
        assert np.array_equal(_bits(view), _bits(want[:, 8:13]))
    one = n.output(buf, 1, batch, coff=Cn - 1).cpu().numpy()                                     # a one-channel view at an odd offset
    assert np.array_equal(_bits(one), _bits(want[:, Cn - 1:Cn]))
