"""Ray families, occupancy grids and parameter cases for the ER-NeRF march kernels, shared by the CPU tier (test_ernerf_loop_cases_host.py) and the
GPU tier (test_ernerf_loop_kernels.py); and the look-ahead walk of k_loop_march (csrc/mf_nerf.hip, loop_march_block) restated in float32 numpy.

A case is one launch: a ray set of 613 rays that holds every family below (61 rays each, labelled in `fam`; the alive list is a permutation, so the
families sit side by side in a wave), one grid, one set of march parameters, n_step and n_alive.  613 = 2 * 256 + 101: the third block is ragged.

Families (b = bound, the box is aabb_infer = b * [-1, -1/2, -1, 1, 1/2, 1], renderer.py:86-89):
  scene       the _scene family of test_ernerf.py (origins near z = -2.2 b, dz > 0, all hit): the control
  octants     all eight sign octants of rays_d, origins on every side of the box
  axis        axis-parallel, the other two components exactly +0.0 / -0.0 (signf_(-0.0) = -1, 1 / d = +-inf)
  axis_voxel  axis-parallel, the origin's other two coordinates exactly on voxel boundaries m * (k / (H / 2) - 1): with a -0.0 component the exit
              distance of the cell is 0 * inf = NaN and fminf has to drop it
  axis_plane  axis-parallel, one origin coordinate exactly on an aabb plane (0 * inf in the slab test: NaN nears / fars for some)
  inside      origins inside the box (near clamped to min_near)
  occupied    origins inside an occupied cell of level 0, every other one min_near in front of it so that the first position visited lies in the cell
              (inside the box where the grid has none)
  miss        rays that pass beside the box (near = far = FLT_MAX) or leave it behind them
  graze       rays that cut an edge or a corner off: far - near below one step for most
  past_far    rays_t >= far on entry (a third of them rays_t == far)
mode "round2": rays_t and the alive list come from the oracle's composite of a first round (a shuffled subset of its survivors)."""
import functools
from types import SimpleNamespace

import numpy as np

from test_ernerf import FLT_MAX, _bitfield, _morton_np, _scene, o_composite, o_march, o_near_far

f32 = np.float32
FAMILIES = ("scene", "octants", "axis", "axis_voxel", "axis_plane", "inside", "occupied", "miss", "graze", "past_far")
FAM = {k: i for i, k in enumerate(FAMILIES)}
PER_FAMILY, N_RAYS = 61, 613
MIN_NEAR = 0.05
MB = 8                                                     # k_loop_march's look-ahead window
GRIDS = ("empty", "full", "one", "checker", "slabs", "random", "sphere")


def one_voxel(H):
    """the occupied voxel of the "one" grid: inside the box (ny within the middle half), off the centre planes"""
    return H // 2 + 1, H // 2 - 2, H // 2 + 3


def _occupied_fn(kind, H):
    if kind == "empty":
        return lambda lvl, nx, ny, nz: np.zeros(nx.shape, np.uint8)
    if kind == "full":
        return lambda lvl, nx, ny, nz: np.ones(nx.shape, np.uint8)
    if kind == "one":
        vx, vy, vz = one_voxel(H)
        return lambda lvl, nx, ny, nz: ((nx == vx) & (ny == vy) & (nz == vz)).astype(np.uint8)
    if kind == "checker":                                  # single voxels: every window of 8 sequence members mixes occupied and empty cells
        return lambda lvl, nx, ny, nz: ((nx + ny + nz + lvl) % 2).astype(np.uint8)
    if kind == "slabs":                                    # two voxels thick, on voxel boundaries, along each axis
        return lambda lvl, nx, ny, nz: ((nx % 16 < 2) | (ny % 16 < 2) | (nz % 16 < 2)).astype(np.uint8)
    if kind == "random":
        return lambda lvl, nx, ny, nz: (np.random.default_rng(1000 + lvl).random(nx.shape) < 0.3).astype(np.uint8)
    if kind == "sphere":
        c, r = (H - 1) / 2, 0.45 * H / 2
        return lambda lvl, nx, ny, nz: (((nx - c) ** 2 + (ny - c) ** 2 + (nz - c) ** 2) < r * r).astype(np.uint8)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def grid(kind, H, cascades):
    """(bitfield, cells): the Morton-ordered bitfield and up to 4096 occupied cells of level 0 inside the box, [n, 3] (possibly none).
    A grid size that is no power of two (96) has Morton codes up to that of (H - 1, H - 1, H - 1) > H^3: the kernels, the reference's included, index the
    bitfield with them, so such a bitfield is allocated up to the next power of two cubed (one cascade only)."""
    fn = _occupied_fn(kind, H)
    if H & (H - 1) == 0:
        bits = _bitfield(H, cascades, fn)
    else:
        assert cascades == 1
        P = 1 << (H - 1).bit_length()
        n = np.arange(H)
        nx, ny, nz = (a.ravel() for a in np.meshgrid(n, n, n, indexing="ij"))
        flat = np.zeros(P ** 3, np.uint8)
        flat[_morton_np(nx, ny, nz)] = fn(0, nx, ny, nz)
        bits = np.packbits(flat.reshape(-1, 8), axis=1, bitorder="little").reshape(-1)
    n = np.arange(H)
    nx, ny, nz = (a.ravel() for a in np.meshgrid(n, n[H // 4 + 1: 3 * H // 4 - 1], n, indexing="ij"))
    cells = np.stack([nx, ny, nz], 1)[fn(0, nx, ny, nz).astype(bool)]
    if cells.shape[0] > 4096:
        cells = cells[np.random.default_rng(5).permutation(cells.shape[0])[:4096]]
    bits.setflags(write=False)
    return bits, cells


def aabb_of(bound):
    return (np.array([-1, -0.5, -1, 1, 0.5, 1], f32) * f32(bound)).astype(f32)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def make_rays(bound, H, cells, seed):
    """ro, rd [613, 3] float32 and fam [613] (index into FAMILIES)"""
    g = np.random.default_rng(seed)
    b, n = float(bound), PER_FAMILY
    e = np.array([b, b / 2, b])
    m0 = min(1.0, b)                                        # mip bound of level 0
    ro, rd, fam = [], [], []

    def add(name, o, d):
        ro.append(np.asarray(o, np.float64)); rd.append(np.asarray(d, np.float64)); fam.append(np.full(len(o), FAM[name]))

    so, sd, _ = _scene(n + N_RAYS - n * len(FAMILIES), seed, H=8)
    add("scene", so.astype(np.float64) * b, sd)
    signs = np.array([[1 if i >> k & 1 else -1 for k in range(3)] for i in range(8)], np.float64)

    def octant_rays(count):
        s = signs[np.arange(count) % 8]
        target = g.uniform(-0.9, 0.9, (count, 3)) * e
        d = _unit((np.abs(g.standard_normal((count, 3))) + 0.05) * s)
        return target - d * g.uniform(1.5, 3.5, (count, 1)) * b, d
    add("octants", *octant_rays(n))

    def axis_rays(count, zero_sign):
        i = np.arange(count)
        a, sg = i % 3, np.where(i // 3 % 2 == 0, 1.0, -1.0)
        o = g.uniform(-0.9, 0.9, (count, 3)) * e
        d = np.zeros((count, 3))
        for r in range(count):
            c1, c2 = (a[r] + 1) % 3, (a[r] + 2) % 3
            z1, z2 = zero_sign(r)
            d[r, a[r]], d[r, c1], d[r, c2] = sg[r], z1, z2
            o[r, a[r]] = -sg[r] * g.uniform(1.5, 3.0) * b
        return o, d, a, sg
    combos = ((0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0))
    o, d, _, _ = axis_rays(n, lambda r: combos[r // 6 % 4])
    add("axis", o, d)
    # on voxel boundaries of level 0; a -0.0 component makes (boundary - position) * (1 / d) = 0 * -inf for the cell the position lies in
    o, d, a, _ = axis_rays(n, lambda r: combos[(1, 3, 2, 3, 0)[r // 6 % 5]])
    for r in range(n):
        for c in ((a[r] + 1) % 3, (a[r] + 2) % 3):
            k = g.integers(H // 4 + 1, 3 * H // 4 - 1)
            o[r, c] = float(f32(m0) * f32(k / (H / 2) - 1))
    add("axis_voxel", o, d)
    # on aabb planes: (plane - origin) = 0 meets 1 / d = inf in the slab test
    o, d, a, sg = axis_rays(n, lambda r: (0.0, 0.0))
    for r in range(n):
        c1 = (a[r] + 1) % 3
        v = r % 4
        if v == 0:
            o[r, c1], d[r, c1] = e[c1], 0.0
        elif v == 1:
            o[r, c1], d[r, c1] = -e[c1], -0.0
        elif v == 2:
            o[r, a[r]] = -sg[r] * e[a[r]]                   # starts on the face it enters through: near = 0 -> min_near
        else:                                               # the x slab is the first the test looks at: a NaN there stays in `near`
            a2 = 1 + r // 4 % 2
            d[r] = 0.0
            d[r, a2] = sg[r]
            o[r] = g.uniform(-0.9, 0.9, 3) * e
            o[r, a2] = -sg[r] * g.uniform(1.5, 3.0) * b
            o[r, 0], d[r, 0] = (-b, 0.0) if r // 8 % 2 == 0 else (b, -0.0)
    add("axis_plane", o, d)
    add("inside", g.uniform(-0.8, 0.8, (n, 3)) * e, _unit(g.standard_normal((n, 3))))
    o = g.uniform(-0.8, 0.8, (n, 3)) * e
    if cells.shape[0]:
        pick = cells[g.integers(0, cells.shape[0], n)]
        o = m0 * ((pick + 0.5 + g.uniform(-0.3, 0.3, (n, 3))) / H * 2 - 1)
    d = _unit(g.standard_normal((n, 3)))
    o[1::2] -= d[1::2] * MIN_NEAR                           # every other one a step back: its first position, at t = min_near, is the one inside the cell
    add("occupied", o, d)
    o, d = octant_rays(n)
    half = n // 2
    o[:half] = g.uniform(-0.9, 0.9, (half, 3)) * e + d[:half] * g.uniform(3.0, 4.0, (half, 1)) * b     # outside (the box's diagonal is 3 b), the box behind them
    o[half:] = np.stack([g.choice([-3.0, 3.0], n - half) * b, g.uniform(-0.4, 0.4, n - half) * b, g.uniform(-0.9, 0.9, n - half) * b], 1)
    d[half:] = _unit(np.stack([g.normal(0, 0.05, n - half), g.choice([-1.0, 1.0], n - half), g.normal(0, 0.05, n - half)], 1))   # beside it
    add("miss", o, d)
    s = signs[np.arange(n) % 8].copy()
    c = s * e
    for r in range(n):
        if r % 4:
            s[r, r % 4 - 1] = 0.0                           # an edge: the normal has no component along it
            c[r, r % 4 - 1] = g.uniform(-0.8, 0.8) * e[r % 4 - 1]
    nrm = _unit(s)
    rnd = g.standard_normal((n, 3))
    d = _unit(rnd - (rnd * nrm).sum(1, keepdims=True) * nrm)
    p = c - nrm * g.uniform(0.0, 0.004, (n, 1)) * b
    add("graze", p - d * g.uniform(1.5, 3.0, (n, 1)) * b, d)
    add("past_far", *octant_rays(n))
    ro, rd, fam = np.concatenate(ro).astype(f32), np.concatenate(rd).astype(f32), np.concatenate(fam)
    assert ro.shape == (N_RAYS, 3) and rd.shape == (N_RAYS, 3)
    return np.ascontiguousarray(ro), np.ascontiguousarray(rd), fam


def _spec(name, grid_kind, H=128, C=1, bound=1.0, dtg=1 / 256, ms=16, n_step=4, n_alive=None, mode="first"):
    return SimpleNamespace(name=name, grid=grid_kind, H=H, C=C, bound=bound, dt_gamma=dtg, max_steps=ms, n_step=n_step, n_alive=n_alive, mode=mode)


def _specs():
    """Chosen cases, not the full product.  (dt_gamma, max_steps) = (1/32, 64) only varies dt where dt_min = 2 sqrt(3) / 64 < dt_max = 2 sqrt(3) 2^(C-1) / H,
    i.e. H / 2^(C-1) < 64: it goes with H = 32 and with three cascades; (1/32, 1024) varies dt at every size."""
    S = []
    for i, k in enumerate(GRIDS):                                                             # every grid at the production parameters
        S.append(_spec(f"base-{k}", k, n_step=1 + i))
    for k, ns in (("checker", 8), ("random", 3), ("slabs", 5)):                               # dt pinned to dt_min / the clamp sequence at H = 128
        S.append(_spec(f"dtmin-{k}", k, dtg=0.0, ms=1024, n_step=ns))
        S.append(_spec(f"clamp-{k}", k, dtg=1 / 32, ms=1024, n_step=9 - ns))
    for k, ns in (("checker", 6), ("random", 8), ("full", 4)):
        S.append(_spec(f"h32-clamp64-{k}", k, H=32, dtg=1 / 32, ms=64, n_step=ns))
    S += [_spec("h32-slabs", "slabs", H=32, n_step=7), _spec("h32-one", "one", H=32, dtg=0.0, ms=1024, n_step=2),
          _spec("h64-checker", "checker", H=64, dtg=1 / 32, ms=1024, n_step=8), _spec("h64-sphere", "sphere", H=64, n_step=3)]
    S += [_spec("h96-checker", "checker", H=96, n_step=5), _spec("h96-random", "random", H=96, dtg=1 / 32, ms=1024, n_step=8),
          _spec("h96-slabs", "slabs", H=96, dtg=0.0, ms=1024, n_step=2)]
    for C, b in ((2, 2.0), (3, 4.0)):
        S += [_spec(f"c{C}-random", "random", C=C, bound=b, n_step=6), _spec(f"c{C}-checker", "checker", C=C, bound=b, dtg=1 / 32, ms=1024, n_step=8),
              _spec(f"c{C}-slabs", "slabs", C=C, bound=b, dtg=0.0, ms=1024, n_step=3)]
    S += [_spec("c3-clamp64-random", "random", C=3, bound=4.0, dtg=1 / 32, ms=64, n_step=8), _spec("c3-clamp64-checker", "checker", C=3, bound=4.0, dtg=1 / 32, ms=64, n_step=5)]
    for b in (0.5, 0.75):
        S += [_spec(f"b{b}-checker", "checker", bound=b, n_step=4), _spec(f"b{b}-random", "random", H=64, bound=b, dtg=1 / 32, ms=1024, n_step=7)]
    for ns in range(1, 9):                                                                    # every n_step: the slab's r = i / n_step cases
        S.append(_spec(f"nstep{ns}-checker", "checker", dtg=1 / 32, ms=1024, n_step=ns))
    for na, ns in ((1, 8), (255, 3), (256, 8), (257, 5)):                                     # around the 256-lane block
        S.append(_spec(f"alive{na}-random", "random", n_step=ns, n_alive=na))
    S += [_spec("round2-checker", "checker", n_step=8, mode="round2"), _spec("round2-random", "random", dtg=1 / 32, ms=1024, n_step=4, mode="round2"),
          _spec("round2-c2-slabs", "slabs", C=2, bound=2.0, n_step=6, mode="round2")]
    for i, s in enumerate(S):
        s.seed = 100 + i
    assert len({s.name for s in S}) == len(S)
    return S


SPECS = _specs()
NAMES = [s.name for s in SPECS]


def fast_allowed(c):
    """the production rule (mf_nerf_loop_march): one cascade and a power-of-two grid no larger than 128"""
    return c.C == 1 and c.H & (c.H - 1) == 0 and c.H <= 128


def step_bounds(c):
    """(dt_min, dt_max) in the kernels' float operations"""
    dt_max = f32(2) * f32(1.7320508075688772) * f32(1 << (c.C - 1)) / f32(c.H)
    return np.fmin(dt_max, f32(2) * f32(1.7320508075688772) / f32(c.max_steps)), dt_max


_cases = {}


def build_case(ref, name):
    """The case `name` with its rays, near / far (the oracle's), rays_t, alive list and the oracle's march of it (`want`: xyzs, dirs, deltas).  Cached and
    shared: nothing in it may be written to."""
    if name in _cases:
        return _cases[name]
    s = SPECS[NAMES.index(name)]
    c = SimpleNamespace(**vars(s))
    c.bits, cells = grid(s.grid, s.H, s.C)
    c.ro, c.rd, c.fam = make_rays(s.bound, s.H, cells, s.seed)
    c.aabb = aabb_of(s.bound)
    c.nears, c.fars = o_near_far(ref, c.ro, c.rd, c.aabb, MIN_NEAR)
    g = np.random.default_rng(s.seed + 7)
    rays_t = c.nears.copy()
    past = np.nonzero(c.fam == FAM["past_far"])[0]
    rays_t[past] = c.fars[past] + np.where(np.arange(past.size) % 3 == 0, 0, g.uniform(0, 1, past.size)).astype(f32)
    alive = g.permutation(N_RAYS).astype(np.int32)
    if s.mode == "round2":
        # a first round of 2 steps over every ray, thin medium: most rays that found two samples survive it with rays_t moved to the last sample's end
        zeros = np.zeros(N_RAYS, f32)
        _, _, deltas = o_march(ref, 2, alive, rays_t, c.ro, c.rd, s.bound, s.dt_gamma, s.max_steps, s.C, s.H, c.bits, c.nears, c.fars, zeros)
        M = N_RAYS * 2
        acc = dict(weights_sum=zeros.copy(), depth=zeros.copy(), image=np.zeros((N_RAYS, 3), f32), amb_aud_sum=zeros.copy(), amb_eye_sum=zeros.copy(),
                   uncertainty_sum=zeros.copy())
        after, rays_t, _ = o_composite(ref, 2, 1e-4, alive, rays_t, np.full(M, 2.0, f32), np.full((M, 3), 0.5, f32), deltas, np.zeros(M, f32), np.zeros(M, f32),
                                       np.zeros(M, f32), acc)
        c.first_round_moved = int((rays_t != c.nears)[after[after >= 0]].sum())
        alive = g.permutation(after[after >= 0])
        alive = np.ascontiguousarray(alive[: max(1, alive.size * 2 // 3)]).astype(np.int32)
    elif s.n_alive is not None:
        if s.n_alive == 1:                                  # a lone ray, one that crosses the box
            alive = alive[c.fam[alive] == FAM["octants"]]
        alive = np.ascontiguousarray(alive[: s.n_alive])
    c.rays_t, c.alive, c.n_alive = rays_t, alive, alive.size
    c.want = o_march(ref, s.n_step, alive, rays_t, c.ro, c.rd, s.bound, s.dt_gamma, s.max_steps, s.C, s.H, c.bits, c.nears, c.fars, np.zeros(alive.size, f32))
    c.counts = (c.want[2][:, 0] > 0).reshape(c.n_alive, s.n_step).sum(1)
    for a in (c.ro, c.rd, c.nears, c.fars, c.rays_t, c.alive) + tuple(c.want):
        a.setflags(write=False)
    _cases[name] = c
    return c


# ---- the look-ahead walk of loop_march_block, in float32 numpy -----------------------------------------------------------------------
def fmaf(a, b, c):
    """fused multiply-add of float32 arrays, correctly rounded: the product is exact in float64, the sum is rounded to odd there (the low bit of an inexact
    float64 sum is forced to 1), and 53 >= 2 * 24 + 2 bits make the second rounding to float32 the correct one"""
    a, b, c = (np.asarray(v, f32).astype(np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def clampf(x, lo, hi):
    return np.fmin(f32(hi), np.fmax(f32(lo), x)).astype(f32)


def _cell(c, tj, dtj, o, d):
    """the voxel of the position at parameter tj (march_ray_ref's operations in its order): position, cell, mip bound, occupancy bit"""
    H, C, bound = c.H, c.C, f32(c.bound)
    pos = [clampf(fmaf(tj, d[:, k], o[:, k]), -bound, bound) for k in range(3)]
    mx = np.fmax(np.abs(pos[0]), np.fmax(np.abs(pos[1]), np.abs(pos[2])))
    la = np.fmin(f32(C - 1), np.fmax(f32(0), np.frexp(mx)[1].astype(f32))).astype(np.int64)
    lb = np.fmin(f32(C - 1), np.fmax(f32(0), np.frexp(dtj * f32(H) * f32(0.5))[1].astype(f32))).astype(np.int64)
    level = np.maximum(la, lb)
    mip_bound = np.fmin(np.ldexp(f32(1), level.astype(np.int32)).astype(f32), bound)
    mip_rbound = (f32(1) / mip_bound).astype(f32)
    n = [clampf((0.5 * fmaf(p, mip_rbound, f32(1)).astype(np.float64) * float(H)).astype(f32), 0, H - 1).astype(np.int64) for p in pos]
    gi = level * H ** 3 + _morton_np(n[0], n[1], n[2])       # fmaf(level, H3, morton) is exact: below 2^24
    occ = ((c.bits[gi // 8] >> (gi % 8).astype(np.uint8)) & 1).astype(bool)
    return pos, n, mip_bound, occ


def lookahead_walk(c):
    """k_loop_march's walk over case c: windows of MB members of the sequence t_{k+1} = t_k + clamp(t_k dt_gamma, dt_min, dt_max), their occupancy bits taken
    together, then the serial pass with `tt`, the exit parameter of the empty cell being skipped; and the slab write-out.  Returns (xyzs, dirs, deltas) as the
    kernel writes them and per-ray flags: nan_exit (an exit distance of an empty cell it evaluated was NaN), mixed (an empty cell was visited between two
    samples less than MB members apart)."""
    na, ns = c.n_alive, c.n_step
    o, d = c.ro[c.alive], c.rd[c.alive]
    t, far = c.rays_t[c.alive].copy(), c.fars[c.alive]
    bound, dtg, rH = f32(c.bound), f32(c.dt_gamma), f32(1) / f32(c.H)
    dt_min, dt_max = step_bounds(c)
    with np.errstate(all="ignore"):
        rd_inv = (f32(1) / d).astype(f32)
        step, tt = np.zeros(na, np.int64), np.full(na, -FLT_MAX, f32)
        s_t, s_dt = np.zeros((na, ns), f32), np.zeros((na, ns), f32)
        done = ~((t < far) & (step < ns))
        base, last, gap = np.zeros(na, np.int64), np.full(na, -10 ** 9, np.int64), np.zeros(na, bool)
        nan_exit, mixed = np.zeros(na, bool), np.zeros(na, bool)
        while not done.all():
            a = np.nonzero(~done)[0]
            ts, ds, cells = [t[a]], [], []
            for j in range(MB):
                ds.append(clampf(ts[j] * dtg, dt_min, dt_max))
                ts.append((ts[j] + ds[j]).astype(f32))
                cells.append(_cell(c, ts[j], ds[j], o[a], d[a]))
            dn, st, tta = np.zeros(a.size, bool), step[a], tt[a]
            for j in range(MB):
                pos, n, mip_bound, occ = cells[j]
                act = ~dn & ~(ts[j] < tta)
                stop = act & ~((ts[j] < far[a]) & (st < ns))
                dn |= stop
                act &= ~stop
                hit, emp = act & occ, act & ~occ
                r = a[hit]
                s_t[r, st[hit]], s_dt[r, st[hit]] = ts[j][hit], ds[j][hit]
                st = st + hit
                tta = np.where(hit, -FLT_MAX, tta).astype(f32)
                m = base[a] + j
                mixed[r] |= gap[r] & (m[hit] - last[r] < MB)
                last[r], gap[r] = m[hit], False
                gap[a[emp]] = True
                ex = [(fmaf(mip_bound, fmaf((n[k].astype(f32) + f32(0.5) + f32(0.5) * np.copysign(f32(1), d[a, k])) * rH, f32(2), f32(-1)), -pos[k]) * rd_inv[a, k]).astype(f32)
                      for k in range(3)]
                nan_exit[a[emp]] |= (np.isnan(ex[0]) | np.isnan(ex[1]) | np.isnan(ex[2]))[emp]
                skip = (ts[j] + np.fmax(f32(0), np.fmin(ex[0], np.fmin(ex[1], ex[2])))).astype(f32)
                tta = np.where(emp, skip, tta).astype(f32)
            t[a], step[a], tt[a], done[a] = ts[MB], st, tta, dn
            base[a] += MB
        filled = np.arange(ns)[None, :] < step[:, None]
        xyz = np.stack([clampf(fmaf(s_t, d[:, None, k], o[:, None, k]), -bound, bound) for k in range(3)], -1)
        xyzs = np.where(filled[..., None], xyz, f32(0)).astype(f32).reshape(na * ns, 3)
        dirs = np.where(filled[..., None], d[:, None, :], f32(0)).astype(f32).reshape(na * ns, 3)
        deltas = np.where(filled[..., None], np.stack([s_dt, (s_t + s_dt).astype(f32)], -1), f32(0)).astype(f32).reshape(na * ns, 2)
    return (xyzs, dirs, deltas), SimpleNamespace(nan_exit=nan_exit, mixed=mixed, counts=step)


def bits(a):
    """the words of a float32 array, for bitwise comparison (-0.0 != +0.0, NaN payloads count)"""
    return np.ascontiguousarray(a, f32).view(np.uint32)
