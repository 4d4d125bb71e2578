"""CPU tier of the loop-kernel tests: the cases of tests/march_cases.py reach what they are meant to reach, judged on the C oracle's output
(oracle/ernerf_ref.c), and the look-ahead walk of k_loop_march, restated in float32 numpy, reproduces the oracle's samples bit for bit -- the
equivalence the kernel's comment argues (every parameter the reference's loop visits is a member of one occupancy-independent sequence), checked
without a GPU.  These are conditions on the inputs, not measurements: the GPU tier (test_ernerf_loop_kernels.py) means little where they fail."""
import numpy as np
import pytest

import march_cases as mc
from test_ernerf import FLT_MAX, ref   # noqa: F401  (ref is a fixture)

DEGENERATE = ("miss", "past_far")
_walks = {}


def _walk(c):
    if c.name not in _walks:
        _walks[c.name] = mc.lookahead_walk(c)
    return _walks[c.name]


def _fam(c):
    return c.fam[c.alive]


def test_case_list_covers_the_parameters():
    S = mc.SPECS
    assert {s.grid for s in S} == set(mc.GRIDS)
    assert {(s.H, s.C) for s in S} >= {(32, 1), (64, 1), (128, 1), (96, 1), (128, 2), (128, 3)}
    assert {(s.C, s.bound) for s in S} >= {(1, 1.0), (1, 0.5), (1, 0.75), (2, 2.0), (3, 4.0)}
    assert {(s.dt_gamma, s.max_steps) for s in S} == {(1 / 256, 16), (0.0, 1024), (1 / 32, 1024), (1 / 32, 64)}
    assert {s.n_step for s in S} == set(range(1, 9))
    assert {s.n_alive for s in S} == {None, 1, 255, 256, 257}
    for s in S:                                             # both variants wherever the rule allows FAST; H = 96 and the cascades only generic
        assert mc.fast_allowed(s) == (s.C == 1 and s.H in (32, 64, 128))
        if s.dt_gamma == 1 / 32:                            # the clamp must have room: dt_min < dt_max
            lo, hi = mc.step_bounds(s)
            assert lo < hi, s.name
    assert max(mc.grid(s.grid, s.H, s.C)[0].nbytes for s in S if s.H == 96 or s.C == 3) <= 768 * 1024


def test_fmaf_restatement_rounds_once():
    """the numpy fused multiply-add against exact rational arithmetic, on operands picked to sit near float32 ties"""
    from fractions import Fraction
    g = np.random.default_rng(0)
    a = g.standard_normal(4000).astype(np.float32)
    b = g.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32) * np.float32(1 + 2.0 ** -12) + g.choice([0, 2.0 ** -30, -2.0 ** -40], 4000).astype(np.float32)
    a[:3], b[:3], c[:3] = [1 + 2.0 ** -23, 1.0, 3.0], [1 + 2.0 ** -23, 2.0 ** -24, 1 + 2.0 ** -23], [2.0 ** -47, 1.0, 2.0 ** -60]
    got = mc.fmaf(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                       # float(Fraction) and float32(float64) round twice: only used to find the neighbours
        cand = sorted({lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))}, key=lambda v: abs(Fraction(float(v)) - exact))
        d0, d1 = abs(Fraction(float(cand[0])) - exact), abs(Fraction(float(cand[1])) - exact)
        if d0 == d1:                                        # a true tie: to even
            want = cand[0] if (cand[0].view(np.uint32) & 1) == 0 else cand[1]
        else:
            want = cand[0]
        assert got[i] == want, (i, a[i], b[i], c[i], got[i], want)


@pytest.mark.parametrize("name", mc.NAMES)
def test_lookahead_walk_reproduces_the_oracle(ref, name):
    c = mc.build_case(ref, name)
    got, st = _walk(c)
    for g, w, what in zip(got, c.want, ("xyzs", "dirs", "deltas")):
        assert np.array_equal(mc.bits(g), mc.bits(w)), (name, what, int((mc.bits(g) != mc.bits(w)).any(-1).sum()))
    assert np.array_equal(st.counts, c.counts)


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_reaches_what_it_is_meant_to(ref, name):
    c = mc.build_case(ref, name)
    fam, counts, ns = _fam(c), c.counts, c.n_step
    d = c.want[2].reshape(c.n_alive, ns, 2)
    # samples sit in the leading slots of a ray, the rest is zero
    assert ((d[:, :, 0] > 0) == (np.arange(ns)[None, :] < counts[:, None])).all()
    for k in DEGENERATE:
        assert counts[fam == mc.FAM[k]].sum() == 0, k
    if c.grid == "empty":
        assert counts.sum() == 0
        return
    assert counts.sum() > 0
    if c.n_alive >= 255:                                    # (a single ray is whichever the permutation put first)
        hit = [k for k in mc.FAMILIES if k not in DEGENERATE and counts[fam == mc.FAM[k]].sum() > 0]
        want = {"occupied"} if c.grid == "one" else {"scene", "octants", "axis", "inside", "occupied"}
        assert want <= set(hit), (name, hit)
        # each n_step: some ray fills every slot, some ray fewer (a lone voxel of 1/64 holds one sample of a step of 1.7 / 64)
        assert ((counts == ns).any() or (c.grid == "one" and c.H == 128)) and (counts < ns).any()
        if ns > 1 and c.grid != "full":
            assert ((counts > 0) & (counts < ns)).any()
    lo, hi = mc.step_bounds(c)
    if c.dt_gamma == 1 / 32:                                # the clamp engages at both ends and leaves room between
        dts = d[:, :, 0][d[:, :, 0] > 0]
        assert (dts == lo).any() and (dts == hi).any() and ((dts > lo) & (dts < hi)).any(), (name, lo, hi, dts.min(), dts.max())
    if c.mode == "round2":
        assert c.first_round_moved > 50 and c.n_alive > 100 and (c.rays_t[c.alive] != c.nears[c.alive]).sum() > 50


def test_ray_families_are_what_their_names_say(ref):
    c = mc.build_case(ref, "base-checker")
    f = lambda k: c.fam == mc.FAM[k]
    lo, _ = mc.step_bounds(c)
    assert N_SIGNS(c.rd[f("octants")]) == 8 and (c.nears[f("octants")] < FLT_MAX).all()
    assert (c.rd[f("scene")][:, 2] > 0).all()
    for k in ("axis", "axis_voxel", "axis_plane"):
        assert ((c.rd[f(k)] == 0).sum(1) == 2).all() and np.signbit(c.rd[f(k)][c.rd[f(k)] == 0]).any()
    assert np.signbit(c.rd[f("axis")][c.rd[f("axis")] == 0]).sum() not in (0, 2 * mc.PER_FAMILY)        # both +0.0 and -0.0
    assert np.isnan(c.nears[f("axis_plane")]).any() and np.isnan(c.fars[f("axis_plane")]).any()
    assert (c.nears[f("axis_plane")] == np.float32(mc.MIN_NEAR)).any()
    assert not np.isnan(c.nears[~f("axis_plane")]).any() and not np.isnan(c.fars[~f("axis_plane")]).any()
    assert (c.nears[f("inside")] == np.float32(mc.MIN_NEAR)).all() and (c.nears[f("occupied")] == np.float32(mc.MIN_NEAR)).mean() > 0.9
    m = c.nears[f("miss")]
    assert (m == FLT_MAX).sum() >= mc.PER_FAMILY // 2 and ((m < FLT_MAX) & (c.fars[f("miss")] < m)).sum() >= mc.PER_FAMILY // 3
    g = f("graze") & (c.nears < FLT_MAX)
    assert g.sum() > mc.PER_FAMILY // 3 and ((c.fars - c.nears)[g] < lo).mean() > 0.5 and ((c.fars - c.nears)[g] > 0).any()
    p = f("past_far")
    assert (c.rays_t[p] >= c.fars[p]).all() and (c.rays_t[p] == c.fars[p]).any() and (c.rays_t[p] > c.fars[p]).any()


def N_SIGNS(d):
    return len({tuple(np.sign(v).astype(int)) for v in d})


def test_checkerboard_mixes_every_window(ref):
    """at least a quarter of the sampled rays visit an empty cell between two samples less than 8 sequence members apart (rays with at least four slots:
    with fewer a ray seldom holds two samples at all)"""
    seen = 0
    for name in mc.NAMES:
        s = mc.SPECS[mc.NAMES.index(name)]
        if s.grid != "checker" or s.n_step < 4:
            continue
        c = mc.build_case(ref, name)
        st = _walk(c)[1]
        sampled = c.counts > 0
        assert st.mixed[sampled].mean() >= 0.25, (name, float(st.mixed[sampled].mean()))
        seen += 1
    assert seen >= 8


def test_voxel_boundary_rays_meet_a_nan_exit_distance(ref):
    """the kernel's exit-distance expression (recomputed in numpy by the walk) is NaN for rays of the axis_voxel family wherever they cross an empty cell"""
    seen = 0
    for name in mc.NAMES:
        s = mc.SPECS[mc.NAMES.index(name)]
        if s.grid in ("full",) or s.n_alive is not None or s.mode != "first":
            continue
        c = mc.build_case(ref, name)
        st = _walk(c)[1]
        fam = _fam(c)
        assert st.nan_exit[fam == mc.FAM["axis_voxel"]].sum() >= 5, (name, int(st.nan_exit[fam == mc.FAM["axis_voxel"]].sum()))
        assert not st.nan_exit[np.isin(fam, [mc.FAM[k] for k in ("scene", "octants", "inside", "occupied", "graze")])].any()
        seen += 1
    assert seen >= 30
