"""ER-NeRF grid maintenance on the device, second half: the torso occupancy grid's rebuild (mf_nerf_torso_grid_update: sweep, 5 x 5 dilate + EMA, mean)
and `mark_untrained_grid` (mf_nerf_mark_untrained), through `HipTorso`, `HipHeadRenderer` and `HipRenderMixin`.

The sweep's positions are bit-equal to the torch statements of renderer.py:511-514; its alpha is held to the CPU torso oracle within the bound `HipTorso`
already has against the reference golden (tests/test_ernerf.py::test_hip_torso_matches_reference_golden: 3e-4 absolute, the same arithmetic); everything
after the sweep is exact.  mark_untrained is compared with the reference's torch statements and a float64 restatement outside a band of 1e-4 around the
frustum's faces."""
import argparse
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
pytestmark = pytest.mark.gpu

ALPHA_TOL = 3e-4                    # tests/test_ernerf.py:745
DECAY = 0.95
SHRINK = 0.8
ROW = 2                             # the code row under test (not 0)


def _rm():
    d = os.path.join(ROOT, "mere-fusion_amd", "dropin")
    if d not in sys.path:
        sys.path.insert(0, d)
    import _raymarching_face
    return _raymarching_face


def morton3D(coords):
    idx = torch.empty(coords.shape[0], dtype=torch.int32, device="cuda")
    _rm().morton3D(coords.int().contiguous(), coords.shape[0], idx)
    return idx


@pytest.fixture(scope="module")
def oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)


def _geometry():
    from mere_fusion_amd.ernerf.field import grid_geometry
    offsets, pls = grid_geometry(num_levels=16, base_resolution=16, log2_hashmap_size=16, desired_resolution=2048)
    return offsets, float(np.log2(pls))


def _torso_sd(seed, G):
    from mere_fusion_amd import weights as W
    offsets, _ = _geometry()
    return W.make_ernerf_torso_state_dict(int(offsets[-1]), seed, individual_dim=8, grid_size=G)


def _pose():
    """A non-identity camera-to-world pose: a rotation about y and z, and a translation."""
    a, b = 0.3, -0.2
    ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rz = torch.tensor([[math.cos(b), -math.sin(b), 0], [math.sin(b), math.cos(b), 0], [0, 0, 1]])
    p = torch.eye(4)
    p[:3, :3] = ry @ rz
    p[:3, 3] = torch.tensor([0.1, -0.2, 0.3])
    return p[None].float()


def _oracle_alpha(sd, row, xys, pose, G):
    """`forward_torso` at every point, no mask (thresh = -1); the oracle takes code row 0, so it gets a state dict whose row 0 is `row`."""
    from oracle import ernerf_net_ref as NR
    offsets, S = _geometry()
    sd0 = dict(sd)
    sd0["individual_codes_torso"] = sd["individual_codes_torso"][row:row + 1].clone()
    return NR.run_torso(sd0, xys.cpu(), pose.cpu(), 0.0, offsets, S, torso_shrink=SHRINK, thresh=-1.0, grid_size=G)["torso_alpha"].view(-1)


_SWEEPS = {}


@pytest.fixture(scope="module")
def sweeps(lib_built, oracle_lib):
    """sweeps(G): one device rebuild per grid size, made at first use, shared (and left unchanged) by the tests below."""
    def get(G):
        if G not in _SWEEPS:
            _SWEEPS[G] = _sweep(G)
        return _SWEEPS[G]
    yield get
    _SWEEPS.clear()


def _sweep(G):
    from mere_fusion_amd.ernerf.torso import HipTorso
    sd = _torso_sd(5, G)
    g = torch.Generator().manual_seed(17 + G)
    noise = torch.rand(G * G, 2, generator=g).cuda()
    start = torch.rand(G * G, generator=g)                              # values in [0, 1]: start * decay wins in places, the pooled alpha in others
    start[torch.rand(G * G, generator=g) < 0.1] = 1.0
    start = start.cuda()
    pose, code = _pose(), sd["individual_codes_torso"][[ROW]]
    t = HipTorso(sd, torso_shrink=SHRINK, individual_dim=8, grid_size=G, max_pixels=1024)
    grid, raw, xys = start.clone(), torch.empty(G * G, device="cuda"), torch.empty(G * G, 2, device="cuda")
    mean = t.update_density_grid(grid, pose, code, noise, decay=DECAY, raw_out=raw, xys_out=xys)
    return {"G": G, "sd": sd, "torso": t, "noise": noise, "start": start, "grid": grid, "raw": raw, "xys": xys, "mean": mean, "pose": pose, "code": code}


# ---- 1. positions -------------------------------------------------------------------------------------------------------------------------------
def test_sweep_positions_equal_the_torch_statements(sweeps):
    G = 32
    sweep = sweeps(G)
    X = torch.arange(G, dtype=torch.int32, device="cuda")
    xx, yy = torch.meshgrid(X, X, indexing="ij")
    coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1)], dim=-1)
    half_grid_size = 1 / G
    xys = 2 * coords.float() / (G - 1) - 1                                               # renderer.py:511
    xys = xys * (1 - half_grid_size)                                                     # :512
    xys += (sweep["noise"] * 2 - 1) * half_grid_size                                     # :514, the noise given instead of drawn
    got = sweep["xys"]
    assert torch.equal(got, xys), f"{int((got != xys).sum())} of {xys.numel()} coordinates differ, max {float((got - xys).abs().max()):.3e}"


def _one_hot_sd(G, cell):
    """Torso nets whose alpha is 1.001 (a saturated sigmoid) at the centre of `cell` = (x, y) and -0.001 everywhere else, by construction: four ReLU units
    measure |x - x0| and |y - y0| of the shrunk point, a fifth is the constant 1 (through the code input, which is all ones here), and the output is
    K (0.02 - |x - x0| - |y - y0|) with K = 1e4: +200 at the cell, below -240 one cell away (the spacing is 0.8 * 2 / (G - 1) * (1 - 1 / G) >= 0.044)."""
    sd = _torso_sd(5, G)
    pos = lambda c: np.float32(np.float32(np.float32(np.float32(2.0) * np.float32(c)) * (np.float32(1.0) / np.float32(G - 1))) - np.float32(1.0)) \
        * np.float32(1 - 1 / G) * np.float32(SHRINK)
    x0, y0 = float(pos(cell[0])), float(pos(cell[1]))
    w0, w1, w2 = torch.zeros(32, 32 + 34 + 42 + 8), torch.zeros(32, 32), torch.zeros(4, 32)
    X, Y, ONE = 32, 33, 32 + 34 + 42                                                    # input columns: the shrunk x, y (network.py:189-194) and code element 0
    w0[0, X], w0[0, ONE] = 1, -x0
    w0[1, X], w0[1, ONE] = -1, x0
    w0[2, Y], w0[2, ONE] = 1, -y0
    w0[3, Y], w0[3, ONE] = -1, y0
    w0[4, ONE] = 1
    for i in range(5):
        w1[i, i] = 1
    w2[0, :4], w2[0, 4] = -1e4, 1e4 * 0.02
    sd["torso_net.net.0.weight"], sd["torso_net.net.1.weight"], sd["torso_net.net.2.weight"] = w0, w1, w2
    return sd


@pytest.fixture(scope="module")
def one_hot(lib_built):
    """Raw and dilated grids of one-hot alphas at a corner, on an edge and inside (G = 32, cell centres, start grid -1 so the pooled value always wins)."""
    from mere_fusion_amd.ernerf.torso import HipTorso
    G, out = 32, {}
    for cell in ((0, 0), (0, 10), (5, 20), (31, 31)):
        t = HipTorso(_one_hot_sd(G, cell), torso_shrink=SHRINK, individual_dim=8, grid_size=G, max_pixels=1024)
        grid, raw = torch.full((G * G,), -1.0, device="cuda"), torch.empty(G * G, device="cuda")
        t.update_density_grid(grid, _pose(), torch.ones(1, 8), None, decay=DECAY, raw_out=raw)
        out[cell] = (raw.cpu(), grid.cpu())
    return out


def test_sweep_writes_the_transposed_index(one_hot):
    """`indices = coords[:, 1] * G + coords[:, 0]` (renderer.py:510): the alpha of cell (x, y) lands at y * G + x."""
    G = 32
    for (x, y), (raw, _) in one_hot.items():
        hot = torch.nonzero(raw > 0).view(-1).tolist()
        assert hot == [y * G + x], ((x, y), hot)
        assert float(raw[y * G + x]) == pytest.approx(1.001, abs=1e-6)
        assert bool((raw[torch.arange(G * G) != y * G + x] == np.float32(-0.001)).all())


# ---- 2. sweep values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [32, 128])
def test_sweep_alpha_matches_the_torso_oracle(sweeps, G):
    sweep = sweeps(G)
    want = _oracle_alpha(sweep["sd"], ROW, sweep["xys"], sweep["pose"], G)               # meshgrid order: row x * G + y
    got = sweep["raw"].cpu().view(G, G).t().reshape(-1)                                  # the grid holds cell (x, y) at y * G + x
    err = float((got - want).abs().max())
    print(f"torso sweep G={G}: alpha L-inf vs oracle {err:.3e} (bound {ALPHA_TOL:.1e}) over {want.numel()} cells, alpha in [{float(got.min()):.4f}, {float(got.max()):.4f}]")
    assert torch.isfinite(got).all() and float(want.std()) > 0.01
    assert err <= ALPHA_TOL


# ---- 3. everything after the sweep is exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [32, 128])
def test_dilate_ema_mean_are_exact(sweeps, G):
    sweep = sweeps(G)
    raw, start = sweep["raw"], sweep["start"]
    pooled = torch.nn.functional.max_pool2d(raw.view(1, 1, G, G), kernel_size=5, stride=1, padding=2).view(-1)       # renderer.py:522-525
    want = torch.maximum(start * DECAY, pooled)                                                                      # :527
    assert int((want == pooled).sum()) > 8 and int((want == start * DECAY).sum()) > 8                               # both branches of the max are populated
    assert torch.equal(sweep["grid"], want)
    mean32 = np.float32(float(want.double().mean()))
    got = np.float32(float(sweep["mean"]))
    assert sweep["mean"].dtype == torch.float32 and sweep["mean"].dim() == 0 and sweep["mean"].is_cuda
    assert abs(float(got) - float(mean32)) <= float(np.spacing(mean32)), (got, mean32)
    # a second call from the same start: the same bits (fixed summation order), and the sweep is deterministic
    grid, raw2 = start.clone(), torch.empty_like(raw)
    mean2 = sweep["torso"].update_density_grid(grid, sweep["pose"], sweep["code"], sweep["noise"], decay=DECAY, raw_out=raw2)
    assert torch.equal(raw2, raw) and torch.equal(grid, want)
    assert torch.equal(mean2.view(1).view(torch.int32), sweep["mean"].view(1).view(torch.int32))


@pytest.mark.parametrize("cell,count", [((0, 0), 9), ((31, 31), 9), ((0, 10), 15), ((5, 20), 25)])
def test_dilation_known_answers(one_hot, cell, count):
    """5 x 5 window, stride 1, padding 2 with -inf: the padding never wins, so the cells away from the hot one stay -0.001 (not 0) up to the border."""
    G = 32
    _, grid = one_hot[cell]
    g2 = grid.view(G, G)                                                                 # [y, x]
    hot = {(int(x), int(y)) for y, x in torch.nonzero(g2 > 0).tolist()}
    want = {(cell[0] + dx, cell[1] + dy) for dx in range(-2, 3) for dy in range(-2, 3) if 0 <= cell[0] + dx < G and 0 <= cell[1] + dy < G}
    assert len(want) == count and hot == want
    assert bool((g2[g2 > 0] == g2.max()).all()) and float(g2.max()) == pytest.approx(1.001, abs=1e-6)
    assert bool((g2[g2 <= 0] == np.float32(-0.001)).all()) and int((g2 <= 0).sum()) == G * G - count


# ---- 4. two routes, one answer -------------------------------------------------------------------------------------------------------------------
H, BOUND = 32, 1.0
N_AUD, N_POSES = 8, 4


def get_audio_features(features, att_mode, index):
    """utils.py:43-45 for att_mode 0 (the mixin takes this helper from the module that defines the method it stands in front of)."""
    assert att_mode == 0
    return features[[index]]


def _field_sd():
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.field import grid_geometry
    offsets, _ = grid_geometry(desired_resolution=512 * BOUND)
    return W.make_ernerf_field_state_dict(int(offsets[-1]), 3, exp_eye=True)


def _poses(n, seed=7):
    g = torch.Generator().manual_seed(seed)
    out = _pose().repeat(n, 1, 1)
    out[:, :3, 3] += torch.randn(n, 3, generator=g) * 0.05
    return out


class _ReferenceShapedTorsoBase(torch.nn.Module):
    """What `HipRenderMixin` touches of the reference's torso NeRFNetwork / NeRFRenderer, under the reference's names, with the torso branch of
    `update_extra_state` (renderer.py:421-432, 488-537) and `mark_untrained_grid` (:356-416) restated over torch -- the per-operation route.  Its
    `forward_torso` is the CPU torso oracle: arithmetic that shares nothing with the device sweep."""

    def __init__(self, opt, sd, start_torso, grid_size=H, cuda_ray=True):
        super().__init__()
        G = grid_size
        self.opt, self.bound, self.grid_size, self.density_scale, self.min_near = opt, BOUND, G, 1.0, 0.05
        self.cascade, self.cuda_ray, self.torso, self.exp_eye, self.emb, self.att = 1, cuda_ray, True, True, True, 0
        self.test_train, self.smooth_lips, self.train_camera, self.individual_dim, self.individual_dim_torso = False, False, False, 4, 8
        self.density_thresh, self.density_thresh_torso, self.mean_density_torso = 10.0, 0.01, 0.5
        self.mean_density, self.iter_density, self.local_step, self.mean_count, self.ref_marks, self.enc_a = 0, 0, 0, 0, 0, None
        self.individual_codes = torch.nn.Parameter(torch.zeros(4, 4))
        self.register_buffer("density_grid", torch.zeros(1, G ** 3))
        self.register_buffer("density_bitfield", torch.zeros(G ** 3 // 8, dtype=torch.uint8))
        self.register_buffer("density_grid_torso", start_torso.clone())
        self.register_buffer("step_counter", torch.zeros(16, 2, dtype=torch.int32))
        g = torch.Generator().manual_seed(5)
        self.aud_features, self.eye_area, self.poses = torch.randn(N_AUD, 32, generator=g), torch.rand(N_AUD, 1, generator=g), _poses(N_POSES)
        self._sd, self._names = sd, {}
        for k, v in sd.items():
            if k == "density_grid_torso":
                continue
            name = "p_" + k.replace(".", "__")
            self.register_parameter(name, torch.nn.Parameter(v.clone(), requires_grad=False))
            self._names[name] = k

    @property
    def individual_codes_torso(self):
        return self.p_individual_codes_torso

    def state_dict(self, *a, **k):
        sd = super().state_dict(*a, **k)
        return {self._names.get(key, key): v for key, v in sd.items()}

    def encode_audio(self, a):
        return a

    def forward_torso(self, x, poses, c=None):
        row = int(torch.nonzero((self.individual_codes_torso == c).all(1)).view(-1)[0])
        alpha = _oracle_alpha(self._sd, row, x, poses, self.grid_size)
        return alpha.view(-1, 1).to(x.device), None, None

    def run_cuda(self, *a, **k):
        raise AssertionError("the reference's run_cuda was reached: the device loop did not run")

    def render(self, rays_o, rays_d, auds, bg_coords, poses, **kwargs):
        return self.run_cuda(rays_o, rays_d, auds, bg_coords, poses, **kwargs)

    @torch.no_grad()
    def mark_untrained_grid(self, poses, intrinsic, S=64):
        if not self.cuda_ray:
            return
        self.ref_marks += 1
        self.density_grid[_mark_torch(poses, intrinsic, self.grid_size, self.cascade, self.bound, self.density_grid, S) == 0] = -1

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        if not self.cuda_ray:
            return
        dev, G = self.density_bitfield.device, self.grid_size
        rand_idx = random.randint(0, self.aud_features.shape[0] - 1)
        self.encode_audio(get_audio_features(self.aud_features, self.att, rand_idx).to(dev))
        tmp_grid_torso = torch.zeros_like(self.density_grid_torso)
        rand_idx = random.randint(0, self.poses.shape[0] - 1)
        pose = self.poses[[rand_idx]].to(dev)
        ind_code = self.individual_codes_torso[[rand_idx]] if self.opt.ind_dim_torso > 0 else None
        X = torch.arange(G, dtype=torch.int32, device=dev).split(S)
        half_grid_size = 1 / G
        for xs in X:
            for ys in X:
                xx, yy = torch.meshgrid(xs, ys, indexing="ij")
                coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1)], dim=-1)
                indices = (coords[:, 1] * G + coords[:, 0]).long()
                xys = 2 * coords.float() / (G - 1) - 1
                xys = xys * (1 - half_grid_size)
                xys += (torch.rand_like(xys) * 2 - 1) * half_grid_size
                alphas, _, _ = self.forward_torso(xys, pose, ind_code)
                tmp_grid_torso[indices] = alphas.squeeze(1).float()
        tmp_grid_torso = torch.nn.functional.max_pool2d(tmp_grid_torso.view(1, 1, G, G), kernel_size=5, stride=1, padding=2).view(-1)
        self.density_grid_torso = torch.maximum(self.density_grid_torso * decay, tmp_grid_torso)
        self.mean_density_torso = torch.mean(self.density_grid_torso).item()
        total_step = min(16, self.local_step)
        if total_step > 0:
            self.mean_count = int(self.step_counter[:total_step, 0].sum().item() / total_step)
        self.local_step = 0


def _net(start_torso, **kw):
    from mere_fusion_amd.ernerf.network import HipRenderMixin
    opt = argparse.Namespace(bound=BOUND, min_near=0.05, exp_eye=True, smooth_lips=False, ind_num=4, ind_dim=4, ind_dim_torso=8, density_thresh=10.0,
                             torso_shrink=SHRINK)
    sd = {**_field_sd(), **_torso_sd(5, kw.get("grid_size", H))}

    class Net(HipRenderMixin, _ReferenceShapedTorsoBase):
        pass
    return Net(opt, sd, start_torso, **kw).cuda().eval()


def _draws(S_blk, G):
    """What the reference's two loops draw from torch's device generator, followed by a probe."""
    for x in torch.arange(G).split(S_blk):
        for y in torch.arange(G).split(S_blk):
            torch.rand(len(x) * len(y), 2, device="cuda")
    return torch.rand(4, device="cuda")


@pytest.mark.parametrize("S_blk", [16, 128])              # 4 blocks of 16^2 / one block (S >= grid_size, the reference's default): two ways the noise is drawn
def test_torso_update_two_routes_one_answer(lib_built, oracle_lib, monkeypatch, S_blk):
    start = torch.rand(H * H, generator=torch.Generator().manual_seed(4))

    def run(dropin):
        monkeypatch.setenv("MF_NERF_DROPIN", dropin)
        m = _net(start)
        m.local_step = 3
        with torch.no_grad():
            m.step_counter[:3, 0] = torch.tensor([10, 20, 31], dtype=torch.int32)
        random.seed(9)
        torch.manual_seed(9)
        m.update_extra_state(decay=DECAY, S=S_blk)
        # the random streams stand where two randint calls and the reference's jitter draws leave them
        probe = (random.random(), torch.rand(4, device="cuda"))
        random.seed(9)
        torch.manual_seed(9)
        want = ((random.randint(0, N_AUD - 1), random.randint(0, N_POSES - 1), random.random())[2], _draws(S_blk, H))
        assert probe[0] == want[0] and torch.equal(probe[1], want[1])
        return m
    ref_m = run("0")
    assert (ref_m.mf_torso_grid_updates, ref_m.mf_grid_updates) == (0, 0)
    m = run("1")
    assert (m.mf_torso_grid_updates, m.mf_grid_updates) == (1, 0)
    assert (m.iter_density, m.local_step, m.mean_count) == (ref_m.iter_density, ref_m.local_step, ref_m.mean_count) == (0, 0, 20)
    assert isinstance(m.mean_density_torso, float) and m.density_grid_torso.is_cuda
    diff = float((m.density_grid_torso - ref_m.density_grid_torso).abs().max())
    print(f"two routes (S={S_blk}): density_grid_torso L-inf {diff:.3e}, mean {m.mean_density_torso:.6f} vs {ref_m.mean_density_torso:.6f} (bound {ALPHA_TOL:.1e})")
    assert float(ref_m.density_grid_torso.std()) > 0.01
    assert diff <= ALPHA_TOL                                                              # max and * decay <= 1 are 1-Lipschitz: the sweep's bound carries through
    assert abs(m.mean_density_torso - ref_m.mean_density_torso) <= ALPHA_TOL


# ---- 5. the rebuilt grid is the one rendered ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("update_route", ["1", "0"])
def test_rebuilt_torso_grid_is_the_one_rendered(lib_built, oracle_lib, monkeypatch, update_route):
    from mere_fusion_amd import weights as W
    Wd = 16
    n = Wd * Wd
    ro, rd = W.make_ernerf_camera_rays(Wd)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u = (torch.arange(Wd, dtype=torch.float32) + 0.5) / Wd * 2 - 1
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    bg_coords = torch.stack([xx, yy], -1).reshape(1, n, 2).cuda()
    bg = torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).cuda()
    pose = _pose().cuda()

    def frame(m):
        return m.render(cu(ro)[None], cu(rd)[None], torch.randn(1, 32, device="cuda"), bg_coords, pose, eye=torch.tensor([[0.4]], device="cuda"),
                        bg_color=bg, dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)["image"].view(n, 3)
    monkeypatch.setenv("MF_NERF_DROPIN", "1")
    m = _net(torch.zeros(H * H))                     # the head's bitfield is empty: the image is the torso over the background
    before = frame(m)
    assert m.mf_frames == 1 and torch.equal(before, bg)                                   # an all-zero torso grid under the threshold 0.01: the mask is empty
    monkeypatch.setenv("MF_NERF_DROPIN", update_route)
    random.seed(9)
    torch.manual_seed(9)
    m.update_extra_state(decay=DECAY)
    assert m.mf_torso_grid_updates == (1 if update_route == "1" else 0)
    monkeypatch.setenv("MF_NERF_DROPIN", "1")
    after = frame(m)
    assert m.mf_frames == 2
    grid, thresh = m.density_grid_torso, min(m.density_thresh_torso, m.mean_density_torso)
    assert thresh > 0 and float(grid.max()) > thresh
    explicit = m._mf["renderer"].torso.run_torso(bg_coords, pose, bg, density_grid=grid)
    assert torch.equal(after, explicit["bg_color"])
    occ = torch.nn.functional.grid_sample(grid.view(1, 1, H, H), bg_coords.view(1, n, 1, 2), align_corners=True).view(-1)     # renderer.py:326
    inside, alpha = occ > thresh + 1e-5, explicit["torso_alpha"].view(-1)
    assert int(inside.sum()) > n // 4
    assert bool((alpha[inside] != 0).all()) and bool((alpha[occ < thresh - 1e-5] == 0).all())
    shown = inside & (alpha > 1e-3)
    assert int(shown.sum()) > n // 8 and bool((after[shown] != bg[shown]).any(1).all())


def test_render_with_the_torso_grid_only_in_the_state_dict(lib_built, monkeypatch):
    """A module that carries `density_grid_torso` in its state dict but not as an attribute (the benchmark's reference-shaped stand-in) renders over the grid the
    torso was built from."""
    from mere_fusion_amd import weights as W
    monkeypatch.setenv("MF_NERF_DROPIN", "1")
    Wd = 16
    n = Wd * Wd
    ro, rd = W.make_ernerf_camera_rays(Wd)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    u = (torch.arange(Wd, dtype=torch.float32) + 0.5) / Wd * 2 - 1
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    bg_coords = torch.stack([xx, yy], -1).reshape(1, n, 2).cuda()
    bg = torch.rand(n, 3, generator=torch.Generator().manual_seed(3)).cuda()
    pose = _pose().cuda()
    blob = _torso_sd(5, H)["density_grid_torso"]
    m = _net(blob)
    del m._buffers["density_grid_torso"]
    m.register_parameter("p_density_grid_torso", torch.nn.Parameter(blob.clone().cuda(), requires_grad=False))
    m._names["p_density_grid_torso"] = "density_grid_torso"
    assert not hasattr(m, "density_grid_torso") and "density_grid_torso" in m.state_dict()
    img = m.render(cu(ro)[None], cu(rd)[None], torch.randn(1, 32, device="cuda"), bg_coords, pose, eye=torch.tensor([[0.4]], device="cuda"), bg_color=bg,
                   dt_gamma=1 / 256, max_steps=16, T_thresh=1e-4)["image"].view(n, 3)
    want = m._mf["renderer"].torso.run_torso(bg_coords, pose, bg, density_grid=blob.cuda())
    assert m.mf_frames == 1 and torch.equal(img, want["bg_color"])
    assert 0.05 < float((want["torso_alpha"] != 0).float().mean()) < 0.95


# ---- 6. mark_untrained ----------------------------------------------------------------------------------------------------------------------------
def _look_at_origin(pos):
    """Camera-to-world pose at `pos`: third rotation column pointing at the origin, first column = up x forward."""
    pos = np.asarray(pos, np.float64)
    f = -pos / np.linalg.norm(pos)
    c0 = np.cross(np.array([0.0, 1.0, 0.0]), f)
    c0 /= np.linalg.norm(c0)
    c1 = np.cross(f, c0)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = c0, c1, f, pos
    return p


def _pose_family(n, r=3.35):
    out = []
    for i in range(n):
        th, ph = 0.7 * math.pi * i / n - 0.6, 0.15 * math.sin(3 * i)
        out.append(_look_at_origin([r * math.sin(th) * math.cos(ph), r * math.sin(ph), r * math.cos(th) * math.cos(ph)]))
    return np.stack(out).astype(np.float32)


FOCAL = 32 / math.tan(math.radians(10.62))
INTRINSIC = (FOCAL, FOCAL, 32.0, 32.0)


def _mark_torch(poses, intrinsic, G, cascade, bound_full, density_grid, S=64):
    """renderer.py:363-414 over the morton3D shim: the count of cameras that see each cell."""
    if isinstance(poses, np.ndarray):
        poses = torch.from_numpy(poses)
    B = poses.shape[0]
    fx, fy, cx, cy = intrinsic
    dev = density_grid.device
    X = torch.arange(G, dtype=torch.int32, device=dev).split(S)
    count = torch.zeros_like(density_grid)
    poses = poses.to(count.device)
    for xs in X:
        for ys in X:
            for zs in X:
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing="ij")
                coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
                indices = morton3D(coords).long()
                world_xyzs = (2 * coords.float() / (G - 1) - 1).unsqueeze(0)
                for cas in range(cascade):
                    bound = min(2 ** cas, bound_full)
                    half_grid_size = bound / G
                    cas_world_xyzs = world_xyzs * (bound - half_grid_size)
                    head = 0
                    while head < B:
                        tail = min(head + S, B)
                        cam_xyzs = cas_world_xyzs - poses[head:tail, :3, 3].unsqueeze(1)
                        cam_xyzs = cam_xyzs @ poses[head:tail, :3, :3]
                        mask_z = cam_xyzs[:, :, 2] > 0
                        mask_x = torch.abs(cam_xyzs[:, :, 0]) < cx / fx * cam_xyzs[:, :, 2] + half_grid_size * 2
                        mask_y = torch.abs(cam_xyzs[:, :, 1]) < cy / fy * cam_xyzs[:, :, 2] + half_grid_size * 2
                        count[cas, indices] += (mask_z & mask_x & mask_y).sum(0).reshape(-1)
                        head += S
    return count


def _slack64(poses, intrinsic, G, cascade, bound_full):
    """float64 on the host: per (cascade, Morton cell) the largest slack over the poses, slack = min(z, kx z + 2h - |x|, ky z + 2h - |y|)."""
    fx, fy, cx, cy = intrinsic
    X = torch.arange(G, dtype=torch.int32, device="cuda")
    xx, yy, zz = torch.meshgrid(X, X, X, indexing="ij")
    coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
    indices = morton3D(coords).long().cpu().numpy()
    world = 2 * coords.cpu().numpy().astype(np.float64) / (G - 1) - 1
    P = np.asarray(poses, np.float64)
    out = np.empty((cascade, G ** 3))
    for cas in range(cascade):
        bound = min(2 ** cas, bound_full)
        h = bound / G
        best = np.full(G ** 3, -np.inf)
        for p in P:
            cam = (world * (bound - h) - p[:3, 3]) @ p[:3, :3]
            s = np.minimum(cam[:, 2], np.minimum(cx / fx * cam[:, 2] + 2 * h - np.abs(cam[:, 0]), cy / fy * cam[:, 2] + 2 * h - np.abs(cam[:, 1])))
            best = np.maximum(best, s)
        out[cas, indices] = best
    return out


def _renderer(G, bound):
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    return HipHeadRenderer(None, torch.zeros(G ** 3 // 8, dtype=torch.uint8, device="cuda"), bound=bound, grid_size=G)


def test_mark_untrained_known_answers(lib_built):
    G = 32
    r = _renderer(G, 1.0)
    X = torch.arange(G, dtype=torch.int32, device="cuda")
    xx, yy, zz = torch.meshgrid(X, X, X, indexing="ij")
    coords = torch.cat([xx.reshape(-1, 1), yy.reshape(-1, 1), zz.reshape(-1, 1)], dim=-1)
    idx = morton3D(coords).long()
    at = lambda x, y, z: int(idx[(x * G + y) * G + z])
    start = torch.rand(1, G ** 3, generator=torch.Generator().manual_seed(1)).cuda() + 0.5
    start[0, at(16, 16, 10)] = -1.0                                                      # in front of the camera, already marked
    grid = start.clone()
    cam_z = 0.5                                                                          # on the +z axis inside the grid, looking at the origin
    pose = torch.from_numpy(_look_at_origin([0, 0, cam_z]).astype(np.float32))[None].cuda()
    ptr = grid.data_ptr()
    r.mark_untrained(grid, pose, INTRINSIC, cascades=1)
    assert grid.data_ptr() == ptr
    world_z = (2 * coords[:, 2].float() / (G - 1) - 1) * (1.0 - 1.0 / G)
    behind = torch.zeros(G ** 3, dtype=torch.bool, device="cuda")
    behind[idx] = world_z > cam_z
    assert int(behind.sum()) > 1000 and bool((grid[0, behind] == -1).all())
    assert float(grid[0, at(16, 16, 16)]) == float(start[0, at(16, 16, 16)]) > 0          # the grid centre is seen
    assert float(grid[0, at(16, 16, 10)]) == -1                                          # a mark that was there stays
    kept = grid != -1
    assert int(kept.sum()) > 100 and torch.equal(grid[kept], start[kept])                # every cell that is not marked keeps its bits
    # no poses: refused by name, nothing marked
    import ctypes as C
    from mere_fusion_amd import _lib
    before = grid.clone()
    with pytest.raises(RuntimeError, match="no poses"):
        r.mark_untrained(grid, torch.empty(0, 4, 4, device="cuda"), INTRINSIC, cascades=1)
    l = _lib.lib()
    assert l.mf_nerf_mark_untrained(C.c_void_p(pose.data_ptr()), 0, *INTRINSIC, 1.0, 1, G, C.c_void_p(grid.data_ptr()), None) == -1
    assert b"at least one pose" in l.mf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(grid, before)


@pytest.mark.parametrize("G,C,bound,B", [(32, 2, 2.0, 5), (32, 3, 4.0, 70)])             # 70 poses: more than one staged chunk of 64, and not a multiple of it
def test_mark_untrained_matches_the_torch_statements(lib_built, G, C, bound, B):
    r = _renderer(G, bound)
    assert r.cascade == C
    poses = _pose_family(B)
    start = torch.rand(C, G ** 3, generator=torch.Generator().manual_seed(2)).cuda()
    grid = start.clone()
    r.mark_untrained(grid, torch.from_numpy(poses).cuda(), INTRINSIC, cascades=C)
    dev = (grid == -1).cpu().numpy()
    tor = (_mark_torch(poses, INTRINSIC, G, C, bound, start) == 0).cpu().numpy()
    slack = _slack64(poses, INTRINSIC, G, C, bound)
    f64 = ~(slack > 0)
    near = np.abs(slack) <= 1e-4
    print(f"mark_untrained (H={G}, C={C}, B={B}): {int(near.sum())} of {near.size} cells ({100 * near.mean():.3f} %) within 1e-4 of a frustum face; "
          f"uncovered {100 * f64.mean():.1f} %; torch vs float64 disagree on {int((tor != f64).sum())} cells, device vs float64 on {int((dev != f64).sum())}")
    assert near.mean() <= 0.001
    assert 0.2 <= f64.mean() <= 0.8
    assert np.array_equal(dev[~near], f64[~near]) and np.array_equal(tor[~near], f64[~near]) and np.array_equal(dev[~near], tor[~near])
    kept = grid != -1
    assert torch.equal(grid[kept], start[kept])


# ---- 7. through the mixin -------------------------------------------------------------------------------------------------------------------------
def test_mixin_mark_untrained_grid(lib_built, oracle_lib, monkeypatch):
    monkeypatch.setenv("MF_NERF_DROPIN", "1")
    poses = _pose_family(5)
    g = torch.Generator().manual_seed(6)

    def fresh(**kw):
        m = _net(torch.zeros(kw.get("grid_size", H) ** 2), **kw)
        with torch.no_grad():
            m.density_grid.copy_(torch.rand(m.density_grid.shape, generator=g))
        return m, m.density_grid.clone(), m.density_grid.data_ptr()
    m, start, ptr = fresh()
    want = start.clone()
    want[_mark_torch(poses, INTRINSIC, H, 1, BOUND, start) == 0] = -1
    m.mark_untrained_grid(poses, INTRINSIC)                                              # an ndarray, as the reference's trainer passes
    assert (m.mf_marks, m.ref_marks) == (1, 0) and m.density_grid.data_ptr() == ptr
    first = m.density_grid.clone()
    with torch.no_grad():
        m.density_grid.copy_(start)
    m.mark_untrained_grid(torch.from_numpy(poses), INTRINSIC)                            # a (host) tensor
    assert (m.mf_marks, m.ref_marks) == (2, 0) and m.density_grid.data_ptr() == ptr
    assert torch.equal(m.density_grid, first) and 0.05 < float((first == -1).float().mean()) < 0.95
    assert float((first != want).float().mean()) <= 0.001                                # the torch statements, up to cells on a frustum face
    # MF_NERF_DROPIN=0 and an unserved grid size take the reference's method
    with torch.no_grad():
        m.density_grid.copy_(start)
    monkeypatch.setenv("MF_NERF_DROPIN", "0")
    m.mark_untrained_grid(poses, INTRINSIC)
    assert (m.mf_marks, m.ref_marks) == (2, 1) and torch.equal(m.density_grid, want)
    monkeypatch.setenv("MF_NERF_DROPIN", "1")
    m16, start16, _ = fresh(grid_size=16)
    m16.mark_untrained_grid(poses, INTRINSIC)
    assert (m16.mf_marks, m16.ref_marks) == (0, 1) and int((m16.density_grid == -1).sum()) > 0
    random.seed(3)
    m16.update_extra_state(decay=DECAY)                                                  # the torso rebuild of an unserved size: the reference's method, too
    assert m16.mf_torso_grid_updates == 0 and float(m16.density_grid_torso.abs().max()) > 0
    # without cuda_ray neither method touches anything
    off, start_off, _ = fresh(cuda_ray=False)
    random.seed(3)
    state = random.getstate()
    off.mark_untrained_grid(poses, INTRINSIC)
    off.update_extra_state(decay=DECAY)
    assert (off.mf_marks, off.ref_marks, off.mf_torso_grid_updates) == (0, 0, 0) and random.getstate() == state
    assert torch.equal(off.density_grid, start_off) and float(off.density_grid_torso.abs().max()) == 0 and off.mean_density_torso == 0.5
