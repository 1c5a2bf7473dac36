"""What tests/test_gpu_ragged_nodes.py and tests/golden/make_golden_ragged_nodes_parent.py share: the geometries of the streaming solver
k_fwd_wave (csrc/sk_wave.hip), seeded coarse increments in its layout, sub-grid tables aimed at every place a per-pair end node can sit,
and the recording of plain solve_fwd's values (the launches that existed before the solvers learnt to keep one node per pair)."""
import numpy as np
import torch

RC = (4, 2, 1, 1)                                               # coarse rows per lane at dyadic 0..3 (Tile<DY>::RC)
GEOMETRIES = ("groups8", "groups32", "fullwave", "multiband")
FLAG_SIMPLE, FLAG_FAST_ONLY = 2, 4


def strip(Mc, Nc, dyadic, elem_size):
    """strip_geom of csrc/sk_internal.h restated: (L lanes per pair, nb bands, NUp 16-byte units per padded row)"""
    rc, cw = RC[dyadic], 16 // elem_size
    nup = (-(-Nc // cw) + 7) // 8 * 8
    logl = 3
    while logl < 6 and (rc << logl) < Mc:
        logl += 1
    L = 1 << logl
    nb = -(-Mc // (L * rc))
    if nb > 1:
        while L > nup and L > 8:
            L >>= 1
        nb = -(-Mc // (L * rc))
    return L, nb, nup


def shapes(geometry, dyadic, elem_size):
    """[(Mc, Nc)] of a geometry: lane groups of 8 / of 32, the full wave with one band, and several bands -- with columns enough that the
    band keeps all 64 lanes (NUp >= 64), with 34 (the lane group shrinks to 16) and with 7 (it shrinks to 8)"""
    rc, cw = RC[dyadic], 16 // elem_size
    if geometry == "multiband":
        return [(64 * rc + 1, 7), (64 * rc + 1, 34), (64 * rc + 1, 64 * cw - 1)]
    Mc = {"groups8": 7, "groups32": 16 * rc + 1, "fullwave": 32 * rc + 1}[geometry]
    return [(Mc, 17), (Mc, 34)]


def expected(geometry, Mc, Nc, dyadic, elem_size):
    """(L, multiband) the geometry is meant to produce -- checked by the tests, so that a shape never silently tests another variant"""
    L, nb, _ = strip(Mc, Nc, dyadic, elem_size)
    want = {"groups8": (8, 1), "groups32": (32, 1), "fullwave": (64, 1)}.get(geometry)
    if want is not None:
        assert (L, nb) == want, (geometry, Mc, Nc, dyadic, elem_size, L, nb)
    else:
        assert nb > 1 and L == (8 if Nc == 7 else 64 if Nc > 34 else 16), (geometry, Mc, Nc, dyadic, elem_size, L, nb)
    return L, nb > 1


def instance(dtype, dyadic, naive, multiband, L):
    """device symbol of k_fwd_wave<T, DY, NAIVE, MULTIBAND, FULLWAVE, EDGES = false, 2> as the launch trace names it"""
    b = lambda v: "Lb%dE" % int(bool(v))
    return "_ZN2sk12_GLOBAL__N_110k_fwd_waveI%sLi%dE%s%s%sLb0ELi2EEEvNS0_10WaveParamsE" % (
        "d" if dtype == torch.float64 else "f", dyadic, b(naive), b(multiband), b(L == 64 and not multiband))


def increments(seed, P, Mc, Nc, dtype, device, ld=None):
    """seeded increments [P, Mc, Nc], a view of rows of `ld` elements (default: whole 128-byte lines; the padding is zero): those of the
    linear kernel on random walks of Mc + 1 and Nc + 1 points in three dimensions (conftest's walk), <x[a + 1] - x[a], y[b + 1] - y[b]>.
    (Independent noise per cell is no static kernel's increment: K then changes sign along the grid, and at a node where it passes
    zero the double-precision oracle itself is further than STREAM_TOL from a long-double solve -- 1.5e-11 at K = -0.003 of a
    257 x 127 grid.)"""
    gen = torch.Generator().manual_seed(seed)
    elem = torch.empty((), dtype=dtype).element_size()
    ld = ld or -(-Nc * elem // 128) * 128 // elem
    dx = torch.randn(P, Mc, 3, generator=gen, dtype=torch.float64) / np.sqrt(3 * (Mc + 1))
    dy = torch.randn(P, Nc, 3, generator=gen, dtype=torch.float64) / np.sqrt(3 * (Nc + 1))
    buf = torch.zeros(P, Mc, ld, dtype=dtype)
    buf[..., :Nc] = torch.einsum("pad,pbd->pab", dx, dy).to(dtype)
    return buf.to(device)[..., :Nc]


def aimed_cells(Mc, Nc, dyadic, elem_size, seed=0, extra=24):
    """int32 [P, 2] of sub-grids (mc, nc) = (len_x - 1, len_y - 1): lengths 1, 2 and the padded one; every row k < RC of a pair's first
    lane, of its last lane and of the last lane of a band; the row on either side of every band boundary; every column q < CW of the
    first and of the last 16-byte unit; the column on either side of every 128-byte line boundary -- all rows against all columns --
    and `extra` random ones"""
    rc, cw = RC[dyadic], 16 // elem_size
    L, nb, _ = strip(Mc, Nc, dyadic, elem_size)
    rows = [0, 1, Mc] + list(range(1, rc + 1)) + [Mc - k for k in range(rc)] + [(L - 1) * rc + 1 + k for k in range(rc)]
    for b in range(1, nb):
        rows += [b * L * rc, b * L * rc + 1]
    cols = [0, 1, Nc] + list(range(1, cw + 1)) + [Nc - q for q in range(cw)]
    for line in range(1, -(-Nc // (8 * cw))):
        cols += [line * 8 * cw, line * 8 * cw + 1]
    rows = sorted(set(v for v in rows if 0 <= v <= Mc))
    cols = sorted(set(v for v in cols if 0 <= v <= Nc))
    g = np.random.default_rng(seed)
    cells = [(m, n) for m in rows for n in cols] + list(zip(g.integers(0, Mc + 1, extra).tolist(), g.integers(0, Nc + 1, extra).tolist()))
    return torch.tensor([cells[i] for i in g.permutation(len(cells))], dtype=torch.int32)


PARENT_PAIRS = 5                                                 # pairs per recorded case: a lane group of 8 holds 8, so some stay idle


def parent_cases():
    """(key, dtype, dyadic, naive, Mc, Nc, flags): one shape per geometry (the multi-band ones: all three), dyadic 0-3, both stencils, both
    precisions, the streaming kernel alone (FAST_ONLY) and the anti-diagonal one (SIMPLE)"""
    out = []
    for dtype in (torch.float64, torch.float32):
        elem = 8 if dtype == torch.float64 else 4
        for dyadic in range(4):
            for naive in (False, True):
                for geometry in GEOMETRIES:
                    todo = shapes(geometry, dyadic, elem)
                    for Mc, Nc in (todo if geometry == "multiband" else todo[(dyadic + naive) % 2:][:1]):
                        for flags, tag in ((FLAG_FAST_ONLY, "fast"), (FLAG_SIMPLE, "simple")):
                            out.append(("%s_d%d_n%d_%dx%d_%s" % ("f64" if elem == 8 else "f32", dyadic, naive, Mc, Nc, tag),
                                        dtype, dyadic, naive, Mc, Nc, flags))
    return out


def case_seed(dyadic, naive, Mc, Nc):
    return 100000 * dyadic + 50000 * int(naive) + 100 * Mc + Nc


def record(lib_module, device="cuda"):
    """{key: values} of plain solve_fwd on the seeded increments of every parent case, through the back-end of `lib_module` (a
    sigkernel_amd._lib: this checkout's or the parent's)"""
    be = lib_module.get_backend()
    rec = {}
    for key, dtype, dyadic, naive, Mc, Nc, flags in parent_cases():
        inc = increments(case_seed(dyadic, naive, Mc, Nc), PARENT_PAIRS, Mc, Nc, dtype, device)
        rec[key] = be.solve_fwd(inc, dyadic, naive, flags=flags).cpu().numpy()
    return rec
