"""ER-NeRF's radiance field, torso branch and audio encoder across the configurations their C API accepts, against float64 (ernerf_numerics.py).

test_ernerf.py runs each net at the one configuration of the golden file on benign inputs; here: every individual_dim / exp_eye packing of the field on both
routes (the fused kernel and MF_NERF_FIELD=gemm), sample counts around the MFMA fragment (16) and the workgroup tile (256), positions on, past and far outside
the box at bounds 1, 2 and 1.5, zero and unnormalised directions, stressed audio / eye / code inputs, the torso's individual_dim x grid_size x route matrix
with coordinates at +-1 and every mask state, and the audio encoder from audio_in_dim 1 to 1024 on both sides of its 64 / 65 route switch.

Gates.  Benign inputs: the fixed gates of test_ernerf.py (field 2e-4 / 6e-2, log sigma 4 x that, torso 3e-4 / 5e-2, audio rtol 2e-5 + atol 2e-6), taken against
float64.  Stress inputs (positions, directions, scaled features): K * REPR * magnitude (ernerf_numerics.field_bounds), K = 3 x the worst first measurement on an
MI355X, written in FIELD_K with the measured value.  Output buffers are longer than the sample count and prefilled with a sentinel: the tail must stay untouched.
Every figure is printed before it is asserted (pytest -s shows them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import ernerf_numerics as EN

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
gpu = pytest.mark.gpu
SENT = -777.25                      # no output of any of the three nets
PAD = 37                            # elements past the sample count in every output buffer
FIELD_TOL = {"bf16x3": 2e-4, "bf16": 6e-2}          # test_ernerf.py::test_hip_field_matches_oracle (log sigma: 4 x)
TORSO_TOL = {"bf16x3": 3e-4, "bf16": 5e-2}          # test_ernerf.py::test_hip_torso_matches_reference_golden
AUDIO_TOL = dict(rtol=2e-5, atol=2e-6)              # test_ernerf.py::test_hip_encode_audio_matches_reference_golden

# K of ernerf_numerics.field_bounds per (route, precision) and output: 3 x the worst first measurement on an MI355X over the stress cases in which kernel and
# reference form the same coordinates (test_hip_field_positions at the power-of-two bounds 1 and 2, test_hip_field_input_stress).  The magnitudes are worst-case
# products of |W| over up to five layers, hundreds of times the values themselves, hence K far below 1.  Measured value and its case in the comment.
FIELD_K = {
    ("fused", "bf16x3"): {"log_sigma": 1.13e-2,    # 3.775e-3, stress enc_a_zero (positions: 3.98e-4)
                          "color": 1.12e-1,        # 3.729e-2, positions bound 2 (max abs error 3.95e-4 on directions of norm 10)
                          "amb_aud": 8.9e-2,       # 2.967e-2, positions bound 1
                          "amb_eye": 4.39e-1},     # 1.464e-1, positions bound 2
    ("fused", "bf16"): {"log_sigma": 7.71e-2,      # 2.570e-2, positions bound 2
                        "color": 2.54e-1,          # 8.455e-2, positions bound 1
                        "amb_aud": 1.63e-1,        # 5.443e-2, positions bound 2
                        "amb_eye": 9.96e-1},       # 3.321e-1, positions bound 2
    ("gemm", "bf16x3"): {"log_sigma": 1.21e-3,     # 4.030e-4, positions bound 2
                         "color": 1.04e-1,         # 3.478e-2, positions bound 2
                         "amb_aud": 1.06e-1,       # 3.522e-2, positions bound 1
                         "amb_eye": 1.66},         # 5.534e-1, positions bound 2
}


@pytest.fixture(scope="module", autouse=True)
def oracle_built():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)


def _note(what, value, gate):
    print(f"[ernerf-configs] {what}: {value:.3e} (gate {gate:.3e})")


# ---- field ---------------------------------------------------------------------------------------------------------------------------------------------
def _geometry(bound):
    from mere_fusion_amd.ernerf.field import grid_geometry
    offsets, pls = grid_geometry(desired_resolution=512 * bound)
    return offsets, float(np.log2(pls))


def _field_sd(bound, seed, nind, eye):
    from mere_fusion_amd import weights as W
    sd = W.make_ernerf_field_state_dict(int(_geometry(bound)[0][-1]), seed, nind, eye)
    return {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in sd.items()}      # as the render tests do: sigma of a trained field's size


def _field_inputs(M, seed, bound, nind, eye):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.5, 1.0]) * bound
    d = torch.randn(M, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    enc_a = torch.randn(1, 32, generator=g)
    c = torch.randn(1, 8, generator=g)[:, :nind] * 0.1 if nind else None
    e = torch.tensor([[0.4]]) if eye else None
    return x, d, enc_a, c, e


_fields = {}


def _field(monkeypatch, route, prec, sd, key, bound=1.0, nind=4, eye=True):
    """one handle per configuration for the module; the route is fixed when the handle is built"""
    from mere_fusion_amd.ernerf.field import HipNeRFField
    k = (route, prec, key, bound, nind, eye)
    if k not in _fields:
        if route == "gemm":
            monkeypatch.setenv("MF_NERF_FIELD", "gemm")
        else:
            monkeypatch.delenv("MF_NERF_FIELD", raising=False)
        _fields[k] = HipNeRFField(sd, bound=bound, individual_dim=nind, exp_eye=eye, precision=prec, max_samples=2048)
    return _fields[k]


def _run_field(f, x, d, enc_a, c, e):
    """mf_nerf_field_forward into sentinel-filled buffers PAD longer than M -> the five outputs [:M] on the CPU in float64; the tails must be untouched"""
    M = x.shape[0]
    dev = lambda t: t.float().contiguous().cuda()
    xd, dd, ea = dev(x), dev(d), dev(enc_a.reshape(-1))
    cd = dev(c.reshape(-1)) if c is not None else None
    outs = [torch.full(((M + PAD) * w,), SENT, device="cuda") for w in (1, 3, 1, 1, 1)]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    from mere_fusion_amd import _lib
    _lib.check(f._lib.mf_nerf_field_forward(f._h, p(xd), p(dd), p(ea), p(cd), float(e.reshape(-1)[0]) if e is not None else 0.0, M, *[p(o) for o in outs],
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mf_nerf_field_forward")
    torch.cuda.synchronize()
    res = []
    for o, w in zip(outs, (1, 3, 1, 1, 1)):
        o = o.cpu()
        assert (o[M * w:] == SENT).all(), f"output {len(res)} written past sample {M}"
        res.append(o[:M * w].reshape(M, w).double())
    return res


def _errors(got, w):
    sig, rgb, aa, ae, un = got
    assert (sig > 0).all() and torch.isfinite(sig).all()
    return {"log_sigma": (torch.log(sig[:, 0]) - w.log_sigma).abs(), "color": (rgb - w.color).abs(), "amb_aud": (aa - w.amb_aud).abs(),
            "amb_eye": (ae - w.amb_eye).abs()}


def _check_field_benign(got, w, prec, eye, what):
    tol = FIELD_TOL[prec]
    err = _errors(got, w)
    err["amb_aud"] = err["amb_aud"] / (1 + w.amb_aud.abs())
    gates = {"log_sigma": 4 * tol, "color": tol, "amb_aud": tol, "amb_eye": tol}
    for k, g in gates.items():
        _note(f"{what} {k}", float(err[k].max()), g)
    for k, g in gates.items():
        assert float(err[k].max()) <= g, (what, k)
    if not eye:
        assert (got[3] == 0).all(), "exp_eye off: ambient_eye must be exactly 0"
    assert (got[4] == EN.LN2_F32).all(), "uncertainty is float32(ln 2) in test mode"


def _check_field_stress(got, w, route, prec, what, assert_gate=True):
    """|got - want| <= K * REPR * mag (+ fp32 rounding) per element; prints the K each output needs"""
    K = FIELD_K[(route, prec)]
    one = EN.field_bounds(w, prec, dict.fromkeys(K, 1.0))
    zero = EN.field_bounds(w, prec, dict.fromkeys(K, 0.0))
    ok = (w.log_sigma > -80) & (w.log_sigma < 80)                          # sigma representable (and normal) in fp32
    sig = got[0][:, 0]
    assert torch.isfinite(sig[ok]).all() and (sig[ok] > 0).all(), what
    for o in got[1:]:
        assert torch.isfinite(o).all(), what
    err = {"log_sigma": torch.where(ok, (torch.log(sig) - w.log_sigma).abs(), torch.zeros_like(sig)), "color": (got[1] - w.color).abs(),
           "amb_aud": (got[2] - w.amb_aud).abs(), "amb_eye": (got[3] - w.amb_eye).abs()}
    need = {}
    for k in K:
        unit = (one[k] - zero[k]).reshape(err[k].shape[0], -1)
        e = (err[k].reshape(unit.shape) - zero[k].reshape(err[k].shape[0], -1)).clamp_min(0)
        need[k] = float(torch.where(unit > 0, e / unit.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e))).max())
        _note(f"{what} K needed for {k} (max abs error {float(err[k].max()):.3e})", need[k], K[k])
    if assert_gate:
        for k in K:
            assert need[k] <= K[k], (what, k, need[k])
    assert (got[4] == EN.LN2_F32).all()
    return need


ROUTES = [("fused", "bf16x3"), ("fused", "bf16"), ("gemm", "bf16x3")]


@gpu
@pytest.mark.parametrize("route,prec", ROUTES, ids=lambda v: v)
@pytest.mark.parametrize("eye", [False, True], ids=["noeye", "eye"])
@pytest.mark.parametrize("nind", [0, 3, 4, 8])
def test_hip_field_configuration_matrix(lib_built, monkeypatch, nind, eye, route, prec):
    """Every packing of sigma's and colour's first layers (36 + 32 + eye, SH 16 + geo 64 + nind) on both routes, M = 300, all five outputs against float64; on
    the gemm route also against the fused kernel on the same inputs."""
    offsets, S = _geometry(1.0)
    sd = _field_sd(1.0, 10 + nind, nind, eye)
    x, d, enc_a, c, e = _field_inputs(300, 20 + nind, 1.0, nind, eye)
    want = EN.field64(sd, x, d, enc_a, c, e, offsets, S, 1.0)
    got = _run_field(_field(monkeypatch, route, prec, sd, "matrix", 1.0, nind, eye), x, d, enc_a, c, e)
    _check_field_benign(got, want, prec, eye, f"matrix nind={nind} eye={eye} {route} {prec}")
    if route == "gemm":
        other = _run_field(_field(monkeypatch, "fused", prec, sd, "matrix", 1.0, nind, eye), x, d, enc_a, c, e)
        tol = FIELD_TOL[prec]
        diffs = {"log_sigma": (torch.log(got[0]) - torch.log(other[0])).abs().max(), "color": (got[1] - other[1]).abs().max(),
                 "amb_aud": ((got[2] - other[2]).abs() / (1 + other[2].abs())).max(), "amb_eye": (got[3] - other[3]).abs().max()}
        for k, v in diffs.items():
            _note(f"matrix nind={nind} eye={eye} gemm vs fused {k}", float(v), 4 * tol if k == "log_sigma" else tol)
        for k, v in diffs.items():
            assert float(v) <= (4 * tol if k == "log_sigma" else tol), k


COUNTS = [("fused", "bf16x3", m) for m in (1, 15, 16, 17, 255, 256, 257, 1023, 1025)] + [("fused", "bf16", m) for m in (16, 17, 257)] + \
         [("gemm", "bf16x3", m) for m in (1, 17, 257)]


@gpu
@pytest.mark.parametrize("route,prec,M", COUNTS, ids=[f"{r}-{p}-{m}" for r, p, m in COUNTS])
def test_hip_field_sample_counts(lib_built, monkeypatch, route, prec, M):
    """Sample counts at and around the 16-sample MFMA fragment, the 256-sample workgroup tile and the 1024-token buffer row: [:M] against float64 (a wrong row of
    a fragment differs by O(1)), [M:] untouched."""
    offsets, S = _geometry(1.0)
    sd = _field_sd(1.0, 3, 4, True)
    x, d, enc_a, c, e = _field_inputs(M, 100 + M, 1.0, 4, True)
    want = EN.field64(sd, x, d, enc_a, c, e, offsets, S, 1.0)
    got = _run_field(_field(monkeypatch, route, prec, sd, "counts"), x, d, enc_a, c, e)
    _check_field_benign(got, want, prec, True, f"counts M={M} {route} {prec}")


def _edge_positions(bound, seed):
    """[M, 3] positions in which every class below stands on every axis alone (the other two coordinates inside the box), in every pair and every triple:
    -bound, +bound, one float outside and inside either, +-2 bound, a cell edge of the coarsest level, the origin (itself a cell edge: 0.5 * 63 + 0.5 = 32)."""
    b = np.float32(bound)
    inf = np.float32(np.inf)
    edge = np.float32(np.float32(19.5 / 63.0) * (2 * b) - b)                 # x01 * 63 + 0.5 = 20 at the coarsest level (scale 63), to the nearest float
    S = np.array([-b, b, np.nextafter(-b, -inf), np.nextafter(-b, inf), np.nextafter(b, inf), np.nextafter(b, -inf), -2 * b, 2 * b, edge, 0.0], np.float32)
    rng = np.random.Generator(np.random.PCG64(seed))
    inside = lambda n: ((rng.random((n, 3)) * 2 - 1) * 0.97 * b).astype(np.float32)
    pts = []
    for a in range(3):
        p = inside(len(S)); p[:, a] = S; pts.append(p)
    for a, bb in ((0, 1), (1, 2), (0, 2)):
        s, t = np.meshgrid(S, S, indexing="ij")
        p = inside(s.size); p[:, a] = s.reshape(-1); p[:, bb] = t.reshape(-1); pts.append(p)
    s, t, u = np.meshgrid(S, S, S, indexing="ij")
    pts.append(np.stack([s.reshape(-1), t.reshape(-1), u.reshape(-1)], -1).astype(np.float32))
    return torch.from_numpy(np.concatenate(pts))


@gpu
@pytest.mark.parametrize("route,prec", ROUTES, ids=lambda v: v)
@pytest.mark.parametrize("bound", [1.0, 2.0, 1.5])
def test_hip_field_positions(lib_built, monkeypatch, bound, route, prec):
    """Positions on the faces of the box, one float to either side, far outside, on cell edges and at the origin, with unit, zero and unnormalised (norm up to 10)
    directions.  A plane with a coordinate outside [0, 1] contributes zero features (the C grid oracle under field64 carries that).

    Bound 1.5 is the case where 1 / (2 bound) is no float: the kernels (field_tile, k_nf_prep) once multiplied by fl(1 / 3) where the reference divides by 3, which
    moved a plane coordinate by one ulp -- 6e-8 x the finest level's 767 cells x a feature difference of up to 2 = 9e-5 on a feature, six times what a (hi, lo) bf16
    pair loses.  This test caught it on an MI355X (bf16x3, K needed at bound 1.5 against the worst at bounds 1 and 2: amb_aud 1.64e-1 against 2.97e-2 fused and
    1.67e-1 against 3.52e-2 gemm, max abs error 9.6e-5 against 1.8e-5; log sigma 1.41e-3 against 4.03e-4 gemm); the kernels now divide, the same bits at every
    power-of-two bound.  The gate is the K measured at bounds 1 and 2 and was not widened for it.  After the change bound 1.5 needs K 1.8e-2 (fused) and
    2.1e-2 (gemm) on amb_aud, max abs error 1.6e-5, and 4.2e-4 / 3.7e-4 on log sigma: as the other bounds."""
    offsets, S = _geometry(bound)
    sd = _field_sd(bound, 5, 4, True)
    x = _edge_positions(bound, 7)
    M = x.shape[0]
    _, d, enc_a, c, e = _field_inputs(M, 31, bound, 4, True)
    d = d * torch.tensor([1.0, 0.0, 10.0, 0.3, 5.0]).repeat(M // 5 + 1)[:M, None]
    want = EN.field64(sd, x, d, enc_a, c, e, offsets, S, bound)
    got = _run_field(_field(monkeypatch, route, prec, sd, "positions", bound), x, d, enc_a, c, e)
    # outside on x: planes xy and xz are zero, so the attention nets see only yz; the reference and the kernels must agree on WHICH planes are out
    _check_field_stress(got, want, route, prec, f"positions bound={bound} {route} {prec}")


STRESS = ["enc_a_zero", "enc_a_x30", "enc_a_channel_100", "eye_0", "eye_1", "eye_-1", "eye_4", "code_x50", "log_sigma_pm20"]


@gpu
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", STRESS)
def test_hip_field_input_stress(lib_built, monkeypatch, case, prec):
    """M = 256 with the audio feature zero, x 30 and with one channel at 100, the eye feature at 0, 1, -1, 4, the individual code x 50, and sigma's output row
    scaled until log sigma spans about [-20, 20]; sigma in log space, every output finite where float64's is representable in fp32."""
    offsets, S = _geometry(1.0)
    sd = _field_sd(1.0, 6, 4, True)
    x, d, enc_a, c, e = _field_inputs(256, 41, 1.0, 4, True)
    key = "stress"
    if case == "enc_a_zero":
        enc_a = torch.zeros_like(enc_a)
    elif case == "enc_a_x30":
        enc_a = enc_a * 30
    elif case == "enc_a_channel_100":
        enc_a = enc_a.clone(); enc_a[0, 11] = 100.0
    elif case.startswith("eye_"):
        e = torch.tensor([[float(case[4:])]])
    elif case == "code_x50":
        c = c * 50
    else:
        span = float(EN.field64(sd, x, d, enc_a, c, e, offsets, S, 1.0).log_sigma.abs().max())
        sd = dict(sd); sd["sigma_net.net.2.weight"] = sd["sigma_net.net.2.weight"].clone(); sd["sigma_net.net.2.weight"][0] *= 20.0 / span
        key = "stress-sigma"
    want = EN.field64(sd, x, d, enc_a, c, e, offsets, S, 1.0)
    if case == "log_sigma_pm20":
        assert 19.9 <= float(want.log_sigma.abs().max()) <= 20.1 and float(want.log_sigma.min()) < -5 and float(want.log_sigma.max()) > 5
    got = _run_field(_field(monkeypatch, "fused", prec, sd, key), x, d, enc_a, c, e)
    _check_field_stress(got, want, "fused", prec, f"stress {case} {prec}")


# ---- torso -----------------------------------------------------------------------------------------------------------------------------------------------
def _torso_geometry():
    from mere_fusion_amd.ernerf.field import grid_geometry
    offs, pls = grid_geometry(num_levels=16, base_resolution=16, log2_hashmap_size=16, desired_resolution=2048)
    return offs, float(np.log2(pls))


def _torso_sd(nind, G):
    """the seeded torso tensors with an occupancy grid that is smooth, nowhere below 0.1 and crosses 0.6 over the whole image, the border included"""
    from mere_fusion_amd import weights as W
    sd = W.make_ernerf_torso_state_dict(int(_torso_geometry()[0][-1]), 4, nind, G)
    u = torch.linspace(-1, 1, G, dtype=torch.float64)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    sd["density_grid_torso"] = (0.6 + 0.5 * torch.sin(3 * xx + 1) * torch.cos(2 * yy - 0.5)).float().reshape(-1)
    return sd


POSE = torch.tensor([[0.98, 0.05, -0.19, 0.05], [-0.03, 0.995, 0.09, -0.02], [0.195, -0.083, 0.977, 0.9], [0.0, 0.0, 0.0, 1.0]])
CORNERS = torch.tensor([[-1.0, 1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, -1.0], [-1.0, 0.3], [0.2, 1.0], [1.0, -0.6], [-0.4, -1.0]])


def _torso_coords(N, seed):
    xy = torch.rand(N, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    xy[:min(N, len(CORNERS))] = CORNERS[:N]
    return xy


_torsos = {}


def _torso(monkeypatch, route, prec, nind, G):
    from mere_fusion_amd.ernerf.torso import HipTorso
    k = (route, prec, nind, G)
    if k not in _torsos:
        if route == "gemm":
            monkeypatch.setenv("MF_TORSO", "gemm")
        else:
            monkeypatch.delenv("MF_TORSO", raising=False)
        sd = _torso_sd(nind, G)
        # torso_shrink 1: coordinates at +-1 plus the deform reach the clamp at [-1, 1] (at the default 0.8 they never do)
        _torsos[k] = (HipTorso(sd, torso_shrink=1.0, individual_dim=nind, grid_size=G, precision=prec, max_pixels=1024), sd)
    return _torsos[k]


def _run_torso(t, xy, pose, bg, thresh, code):
    """mf_nerf_torso_forward into sentinel-filled buffers PAD longer than N -> bg_color [N, 3], torso_alpha [N, 1], deform [N, 2] on the CPU in float64"""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.ernerf.torso import wrapped_anchor_code
    N = xy.shape[0]
    xd = xy.float().contiguous().cuda()
    consts = wrapped_anchor_code(t.anchor_points, pose, code)
    cbuf = (C.c_float * len(consts))(*consts.tolist())
    bgd = bg.float().contiguous().cuda() if torch.is_tensor(bg) else None
    outs = [torch.full(((N + PAD) * w,), SENT, device="cuda") for w in (3, 1, 2)]
    p = lambda v: C.c_void_p(v.data_ptr()) if v is not None else None
    _lib.check(t._lib.mf_nerf_torso_set_grid(t._h, p(t.density_grid)), "mf_nerf_torso_set_grid")
    _lib.check(t._lib.mf_nerf_torso_forward(t._h, p(xd), cbuf, p(bgd), int(bgd is not None and bgd.numel() == 3 * N and bgd.dim() == 2),
                                            float(0.0 if bgd is not None else bg), float(thresh), N, p(outs[0]), p(outs[1]), p(outs[2]),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mf_nerf_torso_forward")
    torch.cuda.synchronize()
    res = []
    for o, w in zip(outs, (3, 1, 2)):
        o = o.cpu()
        assert (o[N * w:] == SENT).all(), f"torso output {len(res)} written past pixel {N}"
        res.append(o[:N * w].reshape(N, w).double())
    return dict(zip(("bg_color", "torso_alpha", "deform"), res))


def _mixed_thresh(sd, G, xy):
    """a threshold that masks some pixels and not others, farther than 1e-4 from every sampled occupancy: there fp32 and float64 grid_sample decide alike"""
    occ = EN.grid_sample64(sd["density_grid_torso"].view(G, G), xy)
    for th in (0.6, 0.55, 0.65, 0.5, 0.7):
        if float((occ - th).abs().min()) > 1e-4:
            return th, occ
    raise AssertionError("no threshold clear of every sampled occupancy")


def _check_torso(got, want, prec, what):
    tol = TORSO_TOL[prec]
    errs = {k: float((got[k] - want[k]).abs().max()) for k in ("bg_color", "torso_alpha", "deform")}
    for k, v in errs.items():
        _note(f"{what} {k}", v, tol)
    for k, v in errs.items():
        assert v <= tol, (what, k)
    assert (got["torso_alpha"][~want["mask"]] == 0).all(), "masked pixels must have alpha == 0 exactly"


TORSO_CONFIGS = [(r, "bf16x3", n, g) for r in ("fused", "gemm") for n in (0, 8) for g in (32, 128)] + [("gemm", "bf16", 8, 128)]


@gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("route,prec,nind,G", TORSO_CONFIGS, ids=[f"{r}-{p}-ind{n}-grid{g}" for r, p, n, g in TORSO_CONFIGS])
def test_hip_torso_matrix(lib_built, monkeypatch, route, prec, nind, G, N):
    """individual_dim x grid_size x route at pixel counts around the 64-pixel tile edge, coordinates at +-1 on both axes (the clamp of the deformed position and
    grid_sample's border), a non-identity pose, an individual code other than row 0, the three background forms and a mixed mask whose every pixel sits more than
    1e-4 from the threshold.  `deform` is compared before the mask: the HIP path runs every pixel."""
    t, sd = _torso(monkeypatch, route, prec, nind, G)
    offs, S = _torso_geometry()
    xy = _torso_coords(N, 50 + N)
    thresh, occ = _mixed_thresh(sd, G, xy)
    margin = float((occ - thresh).abs().min())
    assert margin > 1e-4, margin
    if N > 8:
        assert 0 < int((occ > thresh).sum()) < N, "the mask must be mixed"
    code = sd["individual_codes_torso"][2:3] if nind else None
    bgs = {"per_pixel": torch.rand(N, 3, generator=torch.Generator().manual_seed(N)), "rgb": torch.tensor([0.3, 0.5, 0.7]), "scalar": 0.25}
    for name, bg in bgs.items():
        want = EN.torso64(sd, xy, POSE, bg, offs, S, code, torso_shrink=1.0, thresh=thresh, grid_size=G)
        got = _run_torso(t, xy, POSE, bg, thresh, code)
        _check_torso(got, want, prec, f"torso {route} {prec} ind={nind} G={G} N={N} bg={name}")
    if N > 8:
        x2 = xy.double() + want["deform"]
        assert int((x2.abs() > 1).sum()) > 0, "no deformed position reaches the clamp"


@gpu
@pytest.mark.parametrize("mask", ["all_masked", "none_masked"])
@pytest.mark.parametrize("route", ["fused", "gemm"])
def test_hip_torso_uniform_masks(lib_built, monkeypatch, route, mask):
    """a threshold above every occupancy (alpha == 0 everywhere, the background returned as given) and one below every occupancy (no pixel masked)"""
    t, sd = _torso(monkeypatch, route, "bf16x3", 8, 128)
    offs, S = _torso_geometry()
    xy = _torso_coords(65, 77)
    thresh = 2.0 if mask == "all_masked" else -1.0
    bg = torch.rand(65, 3, generator=torch.Generator().manual_seed(5))
    code = sd["individual_codes_torso"][1:2]
    want = EN.torso64(sd, xy, POSE, bg, offs, S, code, torso_shrink=1.0, thresh=thresh, grid_size=128)
    assert int(want["mask"].sum()) == (0 if mask == "all_masked" else 65)
    got = _run_torso(t, xy, POSE, bg, thresh, code)
    _check_torso(got, want, "bf16x3", f"torso {route} {mask}")
    if mask == "all_masked":
        assert torch.equal(got["bg_color"].float(), bg) and (got["torso_alpha"] == 0).all()
    else:
        assert (got["torso_alpha"] != 0).all()


# ---- audio encoder -----------------------------------------------------------------------------------------------------------------------------------------
def _audio_sd(in_dim, uniform=False):
    from mere_fusion_amd import weights as W
    sd = W.make_ernerf_audio_state_dict(EN.audio_template(in_dim), in_dim)
    if uniform:      # equal attention logits: the convs and the Linear's bias at zero leave softmax(0) = 1/8 per window
        sd = {k: (torch.zeros_like(v) if k.startswith("audio_att_net.attentionConvNet") or k == "audio_att_net.attentionNet.0.bias" else v) for k, v in sd.items()}
    return sd


def _windows(n, in_dim, seed):
    return torch.randn(n, in_dim, 16, generator=torch.Generator().manual_seed(seed))


AUDIO = [(d, 2) for d in (1, 29, 32, 64, 65, 300, 1024)] + [(d, 0) for d in (29, 65, 300)]


@gpu
@pytest.mark.parametrize("in_dim,att", AUDIO, ids=[f"in{d}-att{a}" for d, a in AUDIO])
def test_hip_audio_encoder_widths(lib_built, in_dim, att):
    """audio_in_dim on both sides of the 64 / 65 route switch (64: the largest weight arena the one-launch route copies), widths that are no multiple of the wide
    route's 256 threads, with 8 windows and with one: benign, all-zero, one window x 1e3 (a peaked softmax) and equal attention logits (a uniform one) against
    float64; two calls in a row bit-equal (the `done` counter is reset); the smoothing call with `prev` aliasing the output bit-equal to the torch expression."""
    from mere_fusion_amd import _lib
    from mere_fusion_amd.ernerf.audio import HipAudioEncoder
    n = 8 if att else 1
    sd = _audio_sd(in_dim)
    enc = HipAudioEncoder(sd, att=att)
    a = _windows(n, in_dim, 300 + in_dim)
    peaked = a.clone(); peaked[n // 2] *= 1e3
    cases = [("benign", enc, sd, a), ("zero", enc, sd, torch.zeros_like(a)), ("one_window_x1e3", enc, sd, peaked)]
    if att:
        usd = _audio_sd(in_dim, uniform=True)
        cases.append(("uniform_softmax", HipAudioEncoder(usd, att=att), usd, a))
    for name, h, s, inp in cases:
        want = EN.audio64(s, inp, att).numpy()
        got = h.encode_audio(inp.cuda())
        again = h.encode_audio(inp.cuda())
        err = np.abs(got.cpu().numpy() - want)
        _note(f"audio in_dim={in_dim} att={att} {name}: worst |err| / (atol + rtol |want|)",
              float((err / (AUDIO_TOL["atol"] + AUDIO_TOL["rtol"] * np.abs(want))).max()), 1.0)
        assert got.shape == (1, 32) and np.isfinite(got.cpu().numpy()).all()
        np.testing.assert_allclose(got.cpu().numpy(), want, err_msg=name, **AUDIO_TOL)
        assert torch.equal(got, again), f"{name}: a second call on the handle differs"
        if name == "uniform_softmax":
            np.testing.assert_allclose(want, EN.audio64(s, inp, 0).mean(0, keepdim=True).numpy(), rtol=1e-12, atol=1e-12)    # the case is what it claims to be
    # renderer.py:190-194 inside the launch, prev and the output one buffer, over a few frames
    ad = a.cuda()
    buf = enc.encode_audio(ad).clone()
    ref_t = buf.clone()
    for f in range(3):
        af = (ad * (1.0 + 0.1 * f)).contiguous()
        ref_t = 0.35 * ref_t + (1 - 0.35) * enc.encode_audio(af)
        _lib.check(enc._lib.mf_audio_encoder_forward_smooth(enc._h, C.c_void_p(af.data_ptr()), n, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()),
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)), "mf_audio_encoder_forward_smooth")
        assert torch.equal(buf, ref_t), f"smoothed frame {f}"


# ---- CPU: the float64 references against the fp32 oracle --------------------------------------------------------------------------------------------------
def test_float64_references_match_the_fp32_oracle():
    """field64, torso64 and audio64 restate oracle/ernerf_net_ref.py; on benign inputs the fp32 oracle must sit within 1e-5 relative of them: sigma and the
    attention norm (positive, never cancelled) per element, the signed or possibly small outputs relative to |value| + the output's largest |value| (an fp32 dot
    product is exact relative to its terms, not to a cancelled sum)."""
    from oracle import ernerf_net_ref as NR
    # field, with and without the individual code and the eye feature
    offsets, S = _geometry(1.0)
    for nind, eye in ((4, True), (0, False), (3, True)):
        sd = _field_sd(1.0, 1, nind, eye)
        x, d, enc_a, c, e = _field_inputs(300, 2, 1.0, nind, eye)
        w = EN.field64(sd, x, d, enc_a, c, e, offsets, S, 1.0)
        o = NR.field_forward(sd, x, d, enc_a, c, e, offsets, S)
        scale = lambda t: t.abs() + t.abs().max()
        figs = {"log_sigma": ((torch.log(o[0].double()) - w.log_sigma).abs() / scale(w.log_sigma)).max(),
                "sigma": ((o[0].double() - w.sigma).abs() / w.sigma).max(),
                "color": ((o[1].double() - w.color).abs() / scale(w.color)).max(),
                "amb_aud": ((o[2].double() - w.amb_aud).abs() / w.amb_aud).max(),
                "amb_eye": ((o[3].double() - w.amb_eye).abs() / scale(w.amb_eye).clamp_min(1e-300)).max()}
        for k, v in figs.items():
            _note(f"field64 vs fp32 oracle nind={nind} eye={eye} {k}", float(v), 1e-5)
            assert float(v) <= 1e-5, k
        assert torch.equal(o[4].double(), w.unc)
        if not eye:
            assert (w.amb_eye == 0).all() and (o[3] == 0).all()
    # torso: row 0 of the codes, as the oracle takes it
    offs, St = _torso_geometry()
    for nind, G in ((8, 128), (0, 32)):
        sd = _torso_sd(nind, G)
        xy = _torso_coords(257, 9)
        thresh, occ = _mixed_thresh(sd, G, xy)
        bg = torch.rand(257, 3, generator=torch.Generator().manual_seed(1))
        code = sd["individual_codes_torso"][0:1] if nind else None
        o = NR.run_torso(sd, xy, POSE, bg, offs, St, thresh=thresh, grid_size=G)
        # warped by the oracle's own deform (zero on masked pixels, whose outputs the mask discards): the grid's finest level has 2048 cells across the image, so the
        # 1e-8 by which an fp32 deform differs from float64 would move the features behind it by 2e-5 and the comparison would measure the grid, not the restatement
        w = EN.torso64(sd, xy, POSE, bg, offs, St, code, thresh=thresh, grid_size=G, warp_with=o["deform"])
        assert torch.equal(o["mask"], w["mask"]) and 0 < int(w["mask"].sum()) < 257
        m = w["mask"]
        scale = lambda t: t.abs() + t.abs().max()
        figs = {"deform": ((o["deform"].double() - w["deform"])[m].abs() / scale(w["deform"][m])).max(),
                "torso_alpha": ((o["torso_alpha"].double() - w["torso_alpha"]).abs() / scale(w["torso_alpha"])).max(),
                "bg_color": ((o["bg_color"].double() - w["bg_color"]).abs() / scale(w["bg_color"])).max()}
        for k, v in figs.items():
            _note(f"torso64 vs fp32 oracle ind={nind} G={G} {k}", float(v), 1e-5)
            assert float(v) <= 1e-5, k
    # audio encoder at the golden file's width and two others
    for in_dim, att in ((44, 2), (29, 0), (300, 2)):
        sd = _audio_sd(in_dim)
        a = _windows(8 if att else 1, in_dim, 3)
        w, o = EN.audio64(sd, a, att), NR.encode_audio(sd, a, att).double()
        v = float(((o - w).abs() / (w.abs() + w.abs().max())).max())
        _note(f"audio64 vs fp32 oracle in_dim={in_dim} att={att}", v, 1e-5)
        assert v <= 1e-5
