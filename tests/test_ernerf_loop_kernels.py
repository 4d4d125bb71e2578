"""GPU tier: the two per-round kernels of the device-controlled ER-NeRF loop (k_loop_march<FAST> / generic, k_loop_composite; csrc/mf_nerf.hip) looked at
sample for sample, through the diagnostic entry points mf_nerf_loop_march_debug / mf_nerf_loop_composite_debug.

March: every case of tests/march_cases.py (whose CPU tier, test_ernerf_loop_cases_host.py, shows that the cases reach the look-ahead window, the clamp of dt,
NaN exit distances, every n_step ...) and every kernel variant the production rule allows for it, against three references at once -- the reference-shaped
mf_march_rays, the C oracle, and the reference's own kernel where oracle/_ref holds it -- as uint32 words.  Composite: against mf_composite_rays_triplane on
copies of the same buffers, bit for bit (the same operations on the same device), with the survivor list as a set, the control block restated in Python.
Whole loop: frames over grids that are no smooth sphere, through every route of the head."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import march_cases as mc
from test_ernerf import _field_case, o_near_far, ref   # noqa: F401  (ref is a fixture)
from test_ernerf_reference_kernels import REFDIR

SENTINEL = -12345.678                                        # no kernel output: positions lie in [-4, 4], steps and t in [0, 20]
PAD = 192                                                    # sentinel rows behind n_alive * n_step
_dev_bits = {}


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()                  # (a copy: the shared cases are read-only)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _lib():
    from mere_fusion_amd import _lib as L
    return L


def _bits_dev(c):
    key = (c.grid, c.H, c.C)
    if key not in _dev_bits:
        _dev_bits[key] = _cu(c.bits)
    return _dev_bits[key]


def _words(t):
    return mc.bits(t.cpu().numpy())


def _reference_module():
    """the reference's own raymarching module where the build made it (None elsewhere: the comparison with it is then skipped, the other two stay)"""
    path = os.path.join(REFDIR, "_raymarching_face.so")
    if not os.path.exists(path):
        return None
    import importlib.util
    spec = importlib.util.spec_from_file_location("_raymarching_face", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ref_module():
    return _reference_module()


def _march_debug(c, d, variant):
    """k_loop_march on sentinel-filled outputs; returns (xyzs, dirs, deltas) with PAD rows behind the n_alive * n_step the kernel owns"""
    L = _lib()
    M = c.n_alive * c.n_step
    out = [torch.full((M + PAD, k), SENTINEL, device="cuda") for k in (3, 3, 2)]
    ctl = torch.zeros(16, dtype=torch.int32, device="cuda")
    ctl[:4] = torch.tensor([c.n_alive, c.n_step, c.n_step, M], dtype=torch.int32)
    L.check(L.lib().mf_nerf_loop_march_debug(_p(ctl), _p(d["alive"]), _p(d["rays_t"]), _p(d["ro"]), _p(d["rd"]), mc.N_RAYS, c.bound, c.dt_gamma, c.max_steps, c.C,
                                             c.H, _p(d["bits"]), _p(d["fars"]), _p(out[0]), _p(out[1]), _p(out[2]), variant, L.stream_ptr()),
            "mf_nerf_loop_march_debug")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", mc.NAMES)
def test_loop_march_is_the_reference_bit_for_bit(lib_built, ref, ref_module, name):
    c = mc.build_case(ref, name)
    L = _lib()
    M = c.n_alive * c.n_step
    d = dict(alive=_cu(c.alive), rays_t=_cu(c.rays_t), ro=_cu(c.ro), rd=_cu(c.rd), nears=_cu(c.nears), fars=_cu(c.fars), bits=_bits_dev(c))
    zeros = torch.zeros(c.n_alive, device="cuda")
    # the three references: the C oracle (c.want), mf_march_rays on zeroed outputs with noises = 0, the reference's kernel
    refs = {"oracle": [mc.bits(w) for w in c.want]}
    out = [torch.zeros(M, k, device="cuda") for k in (3, 3, 2)]
    L.check(L.lib().mf_march_rays(c.n_alive, c.n_step, _p(d["alive"]), _p(d["rays_t"]), _p(d["ro"]), _p(d["rd"]), c.bound, c.dt_gamma, c.max_steps, c.C, c.H,
                                  _p(d["bits"]), _p(d["nears"]), _p(d["fars"]), _p(out[0]), _p(out[1]), _p(out[2]), _p(zeros), L.stream_ptr()), "mf_march_rays")
    refs["mf_march_rays"] = [_words(t) for t in out]
    if ref_module is not None:
        out = [torch.zeros(M, k, device="cuda") for k in (3, 3, 2)]
        ref_module.march_rays(c.n_alive, c.n_step, d["alive"], d["rays_t"], d["ro"], d["rd"], c.bound, c.dt_gamma, c.max_steps, c.C, c.H, d["bits"], d["nears"],
                              d["fars"], out[0], out[1], out[2], zeros)
        refs["reference kernel"] = [_words(t) for t in out]
    for tag, r in refs.items():                              # a disagreement among the references is a finding of its own
        for a, b, what in zip(r, refs["oracle"], ("xyzs", "dirs", "deltas")):
            assert np.array_equal(a, b), f"{name}: {tag} and the C oracle disagree on {what} ({int((a != b).any(1).sum())} samples)"
    variants = (0, 1, 2) if mc.fast_allowed(c) else (0, 1)
    sentinel = mc.bits(np.float32(SENTINEL))
    for v in variants:
        got = [_words(t) for t in _march_debug(c, d, v)]
        for g, w, what in zip(got, refs["oracle"], ("xyzs", "dirs", "deltas")):
            bad = (g[:M] != w).any(1)
            assert not bad.any(), f"{name} variant {v}: {what} differs on {int(bad.sum())} of {M} slots (first: slot {int(np.argmax(bad))}, family " \
                                  f"{mc.FAMILIES[c.fam[c.alive[int(np.argmax(bad)) // c.n_step]]]})"
            assert (g[M:] == sentinel).all(), f"{name} variant {v}: {what} written beyond n_alive * n_step"
        # slots past a ray's sample count: exact zeros (+0.0), in all three arrays
        empty = (np.arange(c.n_step)[None, :] >= c.counts[:, None]).reshape(-1)
        assert all((g[:M][empty] == 0).all() for g in got)
    print(f"[loop march] {name}: {c.n_alive} rays x {c.n_step}, variants {variants}, references {sorted(refs)}")


@pytest.mark.gpu
def test_loop_march_debug_refuses(lib_built, ref):
    c = mc.build_case(ref, "h96-checker")
    L = _lib()
    d = dict(alive=_cu(c.alive), rays_t=_cu(c.rays_t), ro=_cu(c.ro), rd=_cu(c.rd), fars=_cu(c.fars), bits=_bits_dev(c))
    out = [torch.full((c.n_alive * 8, k), SENTINEL, device="cuda") for k in (3, 3, 2)]

    def call(n_alive, n_step, variant, H=c.H, cascades=1, max_steps=16, n_rays=mc.N_RAYS):
        ctl = torch.zeros(16, dtype=torch.int32, device="cuda")
        ctl[:2] = torch.tensor([n_alive, n_step], dtype=torch.int32)
        return L.lib().mf_nerf_loop_march_debug(_p(ctl), _p(d["alive"]), _p(d["rays_t"]), _p(d["ro"]), _p(d["rd"]), n_rays, c.bound, c.dt_gamma, max_steps, cascades, H,
                                                _p(d["bits"]), _p(d["fars"]), _p(out[0]), _p(out[1]), _p(out[2]), variant, L.stream_ptr())
    assert call(c.n_alive, 4, 2) == -1 and b"FAST" in L.lib().mf_last_error()          # 96 is no power of two
    assert call(c.n_alive, 4, 2, H=128, cascades=2) == -1
    assert call(c.n_alive, 9, 1) == -1 and b"n_step" in L.lib().mf_last_error()
    assert call(c.n_alive, 0, 1) == -1
    assert call(mc.N_RAYS + 1, 4, 1) == -1
    assert call(c.n_alive, 4, 3) == -1 and call(c.n_alive, 4, 1, H=129) == -1 and call(c.n_alive, 4, 1, max_steps=0) == -1 and call(c.n_alive, 4, 1, cascades=9) == -1
    torch.cuda.synchronize()
    assert all((_words(t) == mc.bits(np.float32(SENTINEL))).all() for t in out)          # nothing was launched
    assert call(c.n_alive, 4, 1, n_rays=0) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bound", [1.0, 0.5, 4.0])
def test_loop_init_near_far_over_all_families(lib_built, ref, bound):
    """mf_near_far_from_aabb (the arithmetic k_loop_init shares: near_far_ray) on misses, negative dz, axis-parallel rays and origins on the box's planes"""
    L = _lib()
    H = 128
    ro, rd, fam = mc.make_rays(bound, H, mc.grid("checker", H, 1)[1], 900 + int(bound * 4))
    aabb = mc.aabb_of(bound)
    want = o_near_far(ref, ro, rd, aabb, mc.MIN_NEAR)
    got = [torch.full((mc.N_RAYS + 64,), SENTINEL, device="cuda") for _ in range(2)]
    d_ro, d_rd, d_aabb = _cu(ro), _cu(rd), _cu(aabb)
    L.check(L.lib().mf_near_far_from_aabb(_p(d_ro), _p(d_rd), _p(d_aabb), mc.N_RAYS, mc.MIN_NEAR, _p(got[0]), _p(got[1]), L.stream_ptr()), "mf_near_far_from_aabb")
    for g, w, what in zip(got, want, ("nears", "fars")):
        g = g.cpu().numpy()
        assert (mc.bits(g[mc.N_RAYS:]) == mc.bits(np.float32(SENTINEL))).all()
        g = g[:mc.N_RAYS]
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), what                                   # NaN by NaN-ness, not payload
        assert np.array_equal(mc.bits(g)[~nan], mc.bits(w)[~nan]), what                 # every other word bitwise
    assert np.isnan(want[0]).any() and (want[0] == np.finfo(np.float32).max).any() and (rd[:, 2] < 0).any()
    assert set(fam[np.isnan(want[0]) | np.isnan(want[1])]) == {mc.FAM["axis_plane"]}


# ---- composite -------------------------------------------------------------------------------------------------------------------
T_THRESH = 1e-4
ALIVE_SENTINEL = -7
ACC = ("weights_sum", "depth", "image", "amb_aud_sum", "amb_eye_sum", "uncertainty_sum")


def _composite_inputs(n_alive, n_step, seed, all_end=False):
    """test_hip_composite_matches_oracle's inputs, with the rays (by their place r in the alive list) of five kinds:
      r % 5 == 0  every slot filled, thin medium: survives
      r % 5 == 1  slot k = r // 5 % n_step empty (k = 0: the first slot), the later slots filled again
      r % 5 == 2  opaque at slot k - 1, so T < T_thresh is met at slot k = r // 5 % n_step (k = 0: weights_sum starts above 1 - T_thresh); k = n_step - 1 ends the
                  ray at its last slot
      r % 5 == 3  weights_sum starts just below 1 - T_thresh (one float32 step): not ended at slot 0
      r % 5 == 4  random slots, 10 % of them empty
    and a whole wave of survivors beside a whole wave of ended rays: [64, 128) | [128, 192), and [512, 576) | [448, 512) at the 512-ray block's edge."""
    rng = np.random.default_rng(seed)
    N = n_alive * 2
    alive = rng.permutation(N).astype(np.int32)[:n_alive]
    rays_t = rng.random(N, np.float32)
    sig = (rng.random((n_alive, n_step), np.float32) * 40).astype(np.float32)
    rgb = rng.random((n_alive, n_step, 3), np.float32)
    dt = (rng.random((n_alive, n_step), np.float32) * 0.03 + 0.001).astype(np.float32)
    ws = np.zeros(N, np.float32)
    edge = np.float32(1) - np.float32(T_THRESH)
    below, above = np.nextafter(edge, np.float32(0)), np.nextafter(edge, np.float32(2))
    assert np.float32(1) - below > np.float32(T_THRESH) or np.float32(1) - np.nextafter(below, np.float32(0)) > np.float32(T_THRESH)
    kind = np.arange(n_alive) % 5
    k = np.arange(n_alive) // 5 % n_step
    for lo, hi, end in ((64, 128, False), (128, 192, True), (448, 512, True), (512, 576, False)):
        if hi <= n_alive:
            kind[lo:hi], k[lo:hi] = (2 if end else 0), 0
    if all_end:
        kind[:], k[:] = 2, 0
    for r in range(n_alive):
        v = alive[r]
        if kind[r] == 0:
            sig[r] = 1.0
        elif kind[r] == 1:
            dt[r, k[r]] = 0
        elif kind[r] == 2:
            if k[r] == 0:
                ws[v] = above
            else:
                sig[r, :k[r]] = 1.0
                sig[r, k[r] - 1] = 1e4
        elif kind[r] == 3:
            ws[v] = below if np.float32(1) - below > np.float32(T_THRESH) else np.nextafter(below, np.float32(0))
        else:
            dt[r, rng.random(n_step) < 0.1] = 0
    deltas = np.stack([dt, np.cumsum(dt, 1) + 0.2], -1).astype(np.float32)
    aa, ae, unc = (rng.random((n_alive, n_step), np.float32) for _ in range(3))
    acc = dict(weights_sum=ws, depth=rng.random(N, np.float32), image=rng.random((N, 3), np.float32), amb_aud_sum=rng.random(N, np.float32),
               amb_eye_sum=rng.random(N, np.float32), uncertainty_sum=rng.random(N, np.float32))
    return SimpleNamespace(alive=alive, rays_t=rays_t, sig=sig, rgb=rgb, deltas=deltas, aa=aa, ae=ae, unc=unc, acc=acc, kind=kind, k=k, N=N)


def _next_round(n_alive, step, N, max_steps):
    """loop_n_step / loop_next_round (csrc/mf_nerf_march.h; renderer.py:246-256) restated: ctl[0..3] of the round to come"""
    n_step = max(min(N // n_alive, 8), 1) if (n_alive > 0 and step < max_steps) else 0
    return [n_alive if n_step else 0, n_step, step + n_step, n_alive * n_step if n_step else 0]


def _run_composites(x, n_alive, n_step, N, max_steps, step_after, rounds):
    """the reference-shaped kernel and the loop's kernel on copies of the same buffers"""
    L = _lib()
    samples = [_cu(a) for a in (x.sig, x.rgb, x.deltas, x.aa, x.ae, x.unc)]
    sig, rgb, deltas, aa, ae, unc = samples
    a_ref, t_ref = _cu(x.alive.copy()), _cu(x.rays_t.copy())
    acc_ref = {k: _cu(v.copy()) for k, v in x.acc.items()}
    L.check(L.lib().mf_composite_rays_triplane(n_alive, n_step, T_THRESH, _p(a_ref), _p(t_ref), _p(sig), _p(rgb), _p(deltas), _p(aa), _p(ae), _p(unc),
                                               *[_p(acc_ref[k]) for k in ACC], L.stream_ptr()), "mf_composite_rays_triplane")
    a_in, t_got = _cu(x.alive.copy()), _cu(x.rays_t.copy())
    a_out = torch.full((n_alive + 64,), ALIVE_SENTINEL, dtype=torch.int32, device="cuda")
    acc_got = {k: _cu(v.copy()) for k, v in x.acc.items()}
    ctl = torch.zeros(16, dtype=torch.int32, device="cuda")
    ctl[:4] = torch.tensor([n_alive, n_step, step_after, n_alive * n_step], dtype=torch.int32)
    ctl[8] = rounds
    L.check(L.lib().mf_nerf_loop_composite_debug(_p(ctl), N, max_steps, T_THRESH, _p(a_in), _p(a_out), _p(t_got), _p(sig), _p(rgb), _p(deltas), _p(aa), _p(ae), _p(unc),
                                                 *[_p(acc_got[k]) for k in ACC], L.stream_ptr()), "mf_nerf_loop_composite_debug")
    torch.cuda.synchronize()
    return dict(a_ref=a_ref.cpu().numpy(), t_ref=t_ref.cpu().numpy(), acc_ref={k: v.cpu().numpy() for k, v in acc_ref.items()}, a_out=a_out.cpu().numpy(),
                t=t_got.cpu().numpy(), acc={k: v.cpu().numpy() for k, v in acc_got.items()}, ctl=ctl.cpu().numpy(), a_in=a_in.cpu().numpy())


def _check_composite(x, r, n_alive, n_step, N, max_steps, step_after, rounds):
    survivors = np.sort(r["a_ref"][r["a_ref"] >= 0])
    count = survivors.size
    assert np.array_equal(np.sort(r["a_out"][:count]), survivors)                        # order is free by contract
    assert (r["a_out"][count:] == ALIVE_SENTINEL).all()
    assert np.array_equal(r["a_in"], x.alive)                                            # the round's own list is read only
    assert np.array_equal(mc.bits(r["t"]), mc.bits(r["t_ref"]))
    for k in ACC:                                                                        # the same operations on the same device
        diff = mc.bits(r["acc"][k]) != mc.bits(r["acc_ref"][k])
        assert not diff.any(), f"{k}: {int(diff.sum())} words differ, max |difference| {np.abs(r['acc'][k] - r['acc_ref'][k]).max():.3e}"
    first_empty = x.alive[x.deltas[:, 0, 0] == 0]
    for k in ACC:                                                                        # nothing blended: the input's bits
        assert np.array_equal(mc.bits(r["acc"][k][first_empty]), mc.bits(x.acc[k][first_empty])), k
    untouched = np.setdiff1d(np.arange(x.N), x.alive)
    for k in ACC:
        assert np.array_equal(mc.bits(r["acc"][k][untouched]), mc.bits(x.acc[k][untouched])), k
    assert np.array_equal(mc.bits(r["t"][untouched]), mc.bits(x.rays_t[untouched]))
    want = _next_round(count, step_after, N, max_steps)
    assert list(r["ctl"][:4]) == want, (list(r["ctl"][:4]), want)
    assert r["ctl"][6] == 0 and r["ctl"][7] == 0
    assert r["ctl"][8] == rounds + (1 if want[1] else 0)
    assert (r["ctl"][9:] == 0).all() and r["ctl"][4] == 0 and r["ctl"][5] == 0
    return count


@pytest.mark.gpu
@pytest.mark.parametrize("n_step", range(1, 9))
@pytest.mark.parametrize("n_alive", [1, 511, 512, 513, 1500])
def test_loop_composite_is_the_reference_shaped_kernel(lib_built, n_alive, n_step):
    x = _composite_inputs(n_alive, n_step, 1000 * n_alive + n_step)
    N = (n_alive, 8 * n_alive, 3 * n_alive + 1)[n_step % 3]
    step_after, rounds, max_steps = 3 + n_step, 2, 64
    r1 = _run_composites(x, n_alive, n_step, N, max_steps, step_after, rounds)
    count = _check_composite(x, r1, n_alive, n_step, N, max_steps, step_after, rounds)
    if n_alive >= 511:
        ended = n_alive - count
        assert count >= 100 and ended >= 100
        a_ref = r1["a_ref"]
        assert (a_ref[64:128] >= 0).all() and (a_ref[128:192] < 0).all()                # a whole wave of survivors beside a whole wave of ended rays
        if n_alive == 1500:
            assert (a_ref[448:512] < 0).all() and (a_ref[512:576] >= 0).all()
        kinds = {(int(kd), int(kk)) for kd, kk, a in zip(x.kind, x.k, a_ref) if a < 0}
        assert {(2, k) for k in range(n_step)} <= kinds                                  # ended at every slot, the last included
        assert (x.deltas[:, 0, 0] == 0).sum() >= 10 and all((x.deltas[:, k, 0] == 0).any() for k in range(n_step))
        assert (a_ref[x.kind == 3] >= 0).any() or n_step > 1                             # just below 1 - T_thresh: slot 0 does not end the ray
    r2 = _run_composites(x, n_alive, n_step, N, max_steps, step_after, rounds)           # again: the same bits, the same survivor set
    assert np.array_equal(np.sort(r2["a_out"]), np.sort(r1["a_out"])) and np.array_equal(r2["ctl"], r1["ctl"])
    assert np.array_equal(mc.bits(r2["t"]), mc.bits(r1["t"])) and all(np.array_equal(mc.bits(r2["acc"][k]), mc.bits(r1["acc"][k])) for k in ACC)


@pytest.mark.gpu
def test_loop_composite_both_endings(lib_built):
    """the loop ends by step >= max_steps with rays alive, and with no survivors: no round is counted, ctl[0..3] are zero but the step count"""
    n_alive, n_step = 700, 3
    x = _composite_inputs(n_alive, n_step, 5)
    r = _run_composites(x, n_alive, n_step, 4 * n_alive, 9, 9, 4)                        # step_after == max_steps
    count = _check_composite(x, r, n_alive, n_step, 4 * n_alive, 9, 9, 4)
    assert count > 100 and list(r["ctl"][:4]) == [0, 0, 9, 0] and r["ctl"][8] == 4
    r = _run_composites(x, n_alive, n_step, 4 * n_alive, 9, 8, 4)                        # one step short of it: a further round
    _check_composite(x, r, n_alive, n_step, 4 * n_alive, 9, 8, 4)
    ns = min(4 * n_alive // count, 8)
    assert list(r["ctl"][:4]) == [count, ns, 8 + ns, ns * count] and r["ctl"][8] == 5
    x = _composite_inputs(n_alive, n_step, 6, all_end=True)
    r = _run_composites(x, n_alive, n_step, 4 * n_alive, 64, 5, 4)
    assert _check_composite(x, r, n_alive, n_step, 4 * n_alive, 64, 5, 4) == 0
    assert list(r["ctl"][:4]) == [0, 0, 5, 0] and r["ctl"][8] == 4


@pytest.mark.gpu
def test_loop_composite_debug_refuses(lib_built):
    L = _lib()
    x = _composite_inputs(64, 2, 1)
    bufs = [_cu(a) for a in (x.alive, x.alive.copy(), x.rays_t, x.sig, x.rgb, x.deltas, x.aa, x.ae, x.unc)] + [_cu(x.acc[k]) for k in ACC]

    def call(head, N=128, max_steps=16):
        ctl = torch.zeros(16, dtype=torch.int32, device="cuda")
        ctl[:len(head)] = torch.tensor(head, dtype=torch.int32)
        return L.lib().mf_nerf_loop_composite_debug(_p(ctl), N, max_steps, T_THRESH, *[_p(b) for b in bufs], L.stream_ptr())
    assert call([129, 2]) == -1 and call([64, 9]) == -1 and call([64, -1]) == -1
    assert call([64, 2, 2, 128, 0, 0, 1]) == -1 and call([64, 2, 2, 128, 0, 0, 0, 1]) == -1                   # a counter that is not at rest
    assert call([64, 2, 2, 128, 0, 0, 0, 0, 0, 0, 8]) == -1 and b"feedback" in L.lib().mf_last_error()        # a pointer the kernel would post through
    assert call([64, 2], N=0) == -1 and call([64, 2], max_steps=0) == -1
    torch.cuda.synchronize()
    assert np.array_equal(bufs[1].cpu().numpy(), x.alive)                                                     # nothing was launched


# ---- whole loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["checker", "slabs", "random"])
def test_whole_loop_on_grids_that_are_no_sphere(lib_built, monkeypatch, kind):
    """One 24 x 24 frame at (dt_gamma, max_steps) = (1/32, 64) over a 32^3 grid (there dt_min = 2 sqrt(3) / 64 < dt_max = 2 sqrt(3) / 32, so the step really
    follows t / 32 along part of a ray; at 128^3 the pair pins it): host loop, device loop with the one-cascade march, with the generic march, with the tail
    kernel running every round, and the batched head -- 1e-6 to the host loop, the same bits among the device routes."""
    from mere_fusion_amd import weights as W
    from mere_fusion_amd.ernerf.field import HipNeRFField
    from mere_fusion_amd.ernerf.renderer import HipHeadRenderer
    H, Wd = 32, 24
    lo, hi = mc.step_bounds(SimpleNamespace(C=1, H=H, max_steps=64))
    assert lo < hi
    sd, offsets, S, _, _, enc_a, c, e = _field_case(8, 3)
    sd = {k: (v * 0.35 if k.startswith("sigma_net.net.2") else v) for k, v in sd.items()}
    ro, rd = W.make_ernerf_camera_rays(Wd)
    r = HipHeadRenderer(HipNeRFField(sd, max_samples=Wd * Wd), _cu(np.array(mc.grid(kind, H, 1)[0])), density_scale=40.0, grid_size=H)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    args = (_cu(ro), _cu(rd), enc_a.cuda(), c.cuda(), e.cuda())
    kw = dict(bg_color=bg, dt_gamma=1 / 32, max_steps=64)
    monkeypatch.delenv("MF_NERF_MARCH", raising=False)
    monkeypatch.delenv("MF_NERF_TAIL_AFTER", raising=False)
    want = r.run_cuda(*args, **kw)
    assert len(want["trace"]) >= 2 and (want["weights_sum"] > 0.5).float().mean().item() > 0.02
    keep = lambda o: {k: o[k].clone() for k in ("image", "depth", "weights_sum")}
    fast = keep(r.run_cuda_device(*args, **kw))
    for k in ("image", "depth", "weights_sum"):
        assert (fast[k] - want[k]).abs().max().item() <= 1e-6, k
    monkeypatch.setenv("MF_NERF_MARCH", "generic")
    generic = keep(r.run_cuda_device(*args, **kw))
    monkeypatch.delenv("MF_NERF_MARCH")
    monkeypatch.setenv("MF_NERF_TAIL_AFTER", "0")
    tail = keep(r.run_cuda_device(*args, **kw))
    monkeypatch.delenv("MF_NERF_TAIL_AFTER")
    frame = dict(rays_o=args[0], rays_d=args[1], enc_a=args[2], ind_code=args[3], eye=args[4], bg_color=bg)
    batch = r.run_cuda_device_batch([frame, frame], dt_gamma=1 / 32, max_steps=64)
    torch.cuda.synchronize()
    for tag, got in (("generic", generic), ("tail", tail), ("batch 0", batch[0]), ("batch 1", batch[1])):
        for k in ("image", "depth", "weights_sum"):
            assert torch.equal(got[k], fast[k]), (tag, k, (got[k] - fast[k]).abs().max().item())
