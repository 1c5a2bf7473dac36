"""Truncated-kernel value regimes: the inputs, the long-double yardstick, its certificates' tools and the case tables of
tests/test_truncated_value_regimes_host.py and tests/test_gpu_truncated_value_regimes.py (test infrastructure: numpy, and mpmath for the
certificates; the paths come from conftest.walk; nothing here imports the product package).

Every other test of k_trunc_sig (csrc/sk_truncated.hip) draws random walks with steps of norm 0.2 .. 0.5 and RBFKernel(1.0), compares
with the fp64 torch restatement -- the same recursion in the same precision -- and divides the error by the max-norm of a whole level.
The families below leave that point of value space, the yardstick is long double, and every error is judged PER PAIR:

    scale       plain kernel: the paths (so the steps) times c, c in {1e-18, 1e-3, 10, 1e3} -- level 8 from 1e-291 to 1e45;
                RBF lift: the points times {1e-3, 3, 10} at sigma 0.8
    offset      X + c, Y + c, c in {1e2, 1e4} (lift: sigma 0.8); the plain kernel also X + c, Y - 3 c
    sigma       RBF lift, sigma in {1e-2, 1e2, 1e6, 1e12}
    drift       RBF lift, sigma 1: Y + s sqrt(3 / D) value_regimes.drift_schedule, s in {5, 15, 30} -- exponents down to -2700: the
                subnormal results, the zeros and the clamp at -800 of exp_nonpos / expm1_nonpos inside trunc_points and its adjoint
    degenerate  one batch: a constant path (the same constant in X and Y: y = x at every node of that pair), a path with repeated points
                in the middle, and a path that stands still after 5 steps (more levels than steps); symmetric rows have y = x throughout
    nonfinite   one NaN, one +inf, one -inf coordinate in one path of X; the same for one path of Y (no yardstick: containment)

THE YARDSTICK (``want_levels``): per pair the level terms k_0 .. k_L and their scales scale[m][pair] = sum over nodes and planes of |R^m|,
by the recursion stated at the top of csrc/sk_truncated.hip in numpy long double (``levels_of_G``: test_truncated_static_host._pair_levels'
recursion on a GIVEN G).  What decides its quality is G:
  * plain kernel: G = <dx_i, dy_j> in long double from the STEPS the kernel is given -- TruncatedSigKernel differences the paths in their
    own dtype, and so do the rows here (``steps_of``); never second differences of <x, y>, which at an offset of 1e4 are wrong by
    1e-12 .. 2e-10 of the level;
  * RBF lift (``lifted_G``): the exponents -|x_i - y_c|^2 / sigma from coordinate differences; the first difference along a row as
    kap_low expm1l(-|dE|) with dE itself from differences, dE(i, c) = -(sum_k (y_{c-1,k} - y_{c,k}) ((x_{i,k} - y_{c,k}) + (x_{i,k} - y_{c-1,k}))) / sigma;
    then the difference across rows.  Subtracting expl values is wrong by 1e-9 of the level at sigma = 1e12.
The GRADIENT yardstick (order 1, ``want_grads``) is the reverse recursion of sk_truncated.hip:90-92 in long double -- Rb^L = w_L,
Rb^m = w_m + exclusive 2-D suffix of G Rb^(m+1), dG = sum_m Rb^m P^(m-1) -- and the chain rule: plain, dx_i = sum_j dG[i][j] dy_j and
through the differencing to the points; lift, the transposed second difference to d / d kap and d kap / d x = -2 (x - y) kap / sigma
from differences.  The host test certifies both: the levels against the same recursion in mpmath at 50 digits, the gradient against
central differences of the level yardstick.

UPSTREAM WEIGHTS of the gradient rows: w[m] = randn / max_pair scale[m], so that EVERY level contributes O(1) to the loss whatever the
steps' size (a level term scales as c^(2m): with weights of ones or randn one level would hide all others away from c = 1).  A level
whose scale is below 1e-300 or not finite gets weight 0 -- its reciprocal is not a double.

Shapes are (A, B, Mp, Np, D) with Mp, Np in POINTS (a plain row's step grid has one row and one column fewer)."""
import functools

import numpy as np

import value_regimes as V
from test_truncated_static_host import _excl_cols, _excl_rows

LD = np.longdouble
L_MAX = 8
ORDER1, GENERAL = "k_trunc_sigILi1ELi2E", "k_trunc_sigILi4ELi1E"      # tests/test_gpu_truncated.py
VALUE_BASE, GRAD_BASE = 1e-12, 1e-10      # README: the truncated kernel's values and gradients
TINY = 2.0 ** -1022
OFFSET_SEEDS = V.OFFSET_SEEDS

# family -> variant ("plain" / "rbf") -> [(parameter label, settings)]
FAMILIES = {
    "scale": {"plain": [("c=%g" % c, {"scale": c}) for c in (1e-18, 1e-3, 10.0, 1e3)],
              "rbf": [("c=%g" % c, {"scale": c, "sigma": 0.8}) for c in (1e-3, 3.0, 10.0)]},
    "offset": {"plain": [("c=%g" % c, {"offset": (c, c)}) for c in (1e2, 1e4)] + [("c=%g,-3c" % c, {"offset": (c, -3 * c)}) for c in (1e2, 1e4)],
               "rbf": [("c=%g" % c, {"offset": (c, c), "sigma": 0.8}) for c in (1e2, 1e4)]},
    "sigma": {"rbf": [("sigma=%g" % s, {"sigma": s}) for s in (1e-2, 1e2, 1e6, 1e12)]},
    "drift": {"rbf": [("s=%g" % s, {"drift": s, "sigma": 1.0}) for s in (5.0, 15.0, 30.0)]},
    "degenerate": {"plain": [("batch", {"degenerate": True})], "rbf": [("batch", {"degenerate": True, "sigma": 0.8})]},
    "nonfinite": {v: [("%s in %s" % (n, s), {"poison": (s, n), "sigma": 0.8}) for s in "XY" for n in ("nan", "+inf", "-inf")] for v in ("plain", "rbf")},
}
MEASURED = ("scale", "offset", "sigma", "drift", "degenerate")      # the families with a yardstick and a recorded restatement distance
POISON = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}
POISON_PATH, POISON_POINT, POISON_COORD = 1, 5, 1
FEW_STEPS = 5


def signed_sigma(L):
    """test_gpu_truncated_static.signed_sigma: level weights of either sign"""
    return np.array([0.5] + [(-1.0) ** m * (1.0 + 0.25 * m) for m in range(1, L + 1)])


# ------------------------------------------------------------------------------------------------------------------- inputs
def inputs(settings, row, seed=0):
    """-> X (A, Mp, D), Y (B, Np, D): numpy fp64 PATHS (fp32-rounded for an fp32 row; Y is X for a symmetric row)"""
    A, B, Mp, Np, D = row["shape"]
    sh = V.shape(A, B, Mp, Np, D, 0, sym=row["op"] == "sym", f32=row["f32"])
    st = {k: v for k, v in settings.items() if k in ("scale", "offset", "drift", "sigma")}
    X, Y, _, _ = V.inputs(st, sh, seed)
    if settings.get("degenerate"):
        X, Y = X.copy(), Y.copy()
        X[0] = X[0, :1]                                  # a constant path
        X[1, Mp // 2:Mp // 2 + 3] = X[1, Mp // 2]        # repeated points: two zero steps in the middle
        X[A - 1, FEW_STEPS:] = X[A - 1, FEW_STEPS]       # FEW_STEPS steps, then it stands still: more levels than steps
        if row["op"] != "sym":
            Y[0] = X[0, :1]                              # the same constant: the pair (0, 0) has x = y at every node
            Y[1, Np // 2:Np // 2 + 3] = Y[1, Np // 2]
    if row["op"] == "sym":
        Y = X
    return X, Y


def poisoned(X, Y, settings):
    """the clean batch with one coordinate of one path replaced -> (X, Y, which side, the path's index)"""
    side, name = settings["poison"]
    X, Y = X.copy(), (Y.copy() if Y is not X else None)
    T = X if side == "X" or Y is None else Y
    p = min(POISON_PATH, T.shape[0] - 1)
    T[p, min(POISON_POINT, T.shape[1] - 2), POISON_COORD] = POISON[name]
    return X, (X if Y is None else Y), side, p


def steps_of(P, f32=False):
    """the differences torch forms, X[:, 1:] - X[:, :-1] in the paths' own dtype, as exact fp64 numbers"""
    P = P.astype(np.float32) if f32 else P
    return (P[:, 1:] - P[:, :-1]).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------- yardstick
def plain_G(dx, dy):
    """<dx_i, dy_j> of one pair's steps in long double"""
    return dx.astype(LD) @ dy.astype(LD).T


def _lift_parts(x, y, sigma):
    """one pair's points -> (E exponents, kap, dEc: E(i, c) - E(i, c - 1) for c >= 1), all from coordinate differences, long double"""
    x, y, s = x.astype(LD), y.astype(LD), LD(sigma)
    e = x[:, None, :] - y[None, :, :]
    E = -(e * e).sum(2) / s
    dy = y[:-1] - y[1:]                                   # y_{c-1} - y_c
    dEc = -((dy[None, :, :] * (e[:, 1:, :] + e[:, :-1, :])).sum(2)) / s
    return E, np.exp(E), dEc


def lifted_G(x, y, sigma):
    """G[i - 1][c - 1] = kap(i, c) - kap(i, c - 1) - kap(i - 1, c) + kap(i - 1, c - 1): (Mp - 1, Np - 1) long double"""
    E, kap, dEc = _lift_parts(x, y, sigma)
    down = dEc <= 0
    D = np.where(down, kap[:, :-1] * np.expm1(np.where(down, dEc, 0)), -kap[:, 1:] * np.expm1(np.where(down, 0, -dEc)))
    return D[1:] - D[:-1]


def levels_of_G(G, L, order):
    """one pair: (k_0 .. k_L, scale_0 .. scale_L) in long double; test_truncated_static_host._pair_levels' recursion on a given G"""
    M, N = G.shape
    R = [[G]]
    ks, mags = [LD(1)], [LD(1)]
    for m in range(1, L + 1):
        ks.append(sum(R[p][q].sum() for p in range(len(R)) for q in range(len(R))))
        mags.append(sum(np.abs(R[p][q]).sum() for p in range(len(R)) for q in range(len(R))))
        if m == L:
            break
        d, dn = len(R), min(m + 1, order)
        nxt = [[None] * dn for _ in range(dn)]
        for p in range(dn):
            for q in range(dn):
                if p == 0 and q == 0:
                    total = np.zeros((M, N), dtype=LD)
                    for pp in range(d):
                        for qq in range(d):
                            total = total + R[pp][qq]
                    nxt[0][0] = G * _excl_rows(_excl_cols(total))
                elif p == 0:
                    col = np.zeros((M, N), dtype=LD)
                    for pp in range(d):
                        col = col + R[pp][q - 1]
                    nxt[0][q] = G * _excl_rows(col) / LD(q + 1)
                elif q == 0:
                    rw = np.zeros((M, N), dtype=LD)
                    for qq in range(d):
                        rw = rw + R[p - 1][qq]
                    nxt[p][0] = G * _excl_cols(rw) / LD(p + 1)
                else:
                    nxt[p][q] = G * R[p - 1][q - 1] / LD((p + 1) * (q + 1))
        R = nxt
    return np.array(ks, dtype=LD), np.array(mags, dtype=LD)


def pair_G(variant, sigma, x, y):
    """one pair's G: plain -- x, y hold STEPS; rbf -- POINTS"""
    return plain_G(x, y) if variant == "plain" else lifted_G(x, y, sigma)


def _pairs(A, B, paired):
    return [(a, a) for a in range(A)] if paired else [(a, b) for a in range(A) for b in range(B)]


def want_levels(variant, sigma, X, Y, L, order=1, paired=False):
    """-> (levels, scale), each (L + 1, A, B) -- paired (L + 1, P) -- long double, PER PAIR.  X, Y: steps (plain) or points (rbf)."""
    A, B = X.shape[0], Y.shape[0]
    pairs = _pairs(A, B, paired)
    lev, scale = np.zeros((L + 1, len(pairs)), dtype=LD), np.zeros((L + 1, len(pairs)), dtype=LD)
    for n, (a, b) in enumerate(pairs):
        lev[:, n], scale[:, n] = levels_of_G(pair_G(variant, sigma, X[a], Y[b]), L, order)
    return (lev, scale) if paired else (lev.reshape(L + 1, A, B), scale.reshape(L + 1, A, B))


def _excl2(T):
    return _excl_rows(_excl_cols(T))


def _suffix2(T):
    return _excl2(T[::-1, ::-1])[::-1, ::-1]


def dG_of(G, w):
    """order 1: d (sum_m w[m - 1] k_m) / dG of one pair, the reverse recursion of sk_truncated.hip:90-92"""
    L = len(w)
    P = [np.ones_like(G)]                       # P^0 = 1, P^m = exclusive 2-D prefix of R^m
    R = G
    for m in range(1, L):
        P.append(_excl2(R))
        R = G * P[m]
    Rb = np.full_like(G, w[L - 1])
    dG = Rb * P[L - 1]
    for m in range(L - 1, 0, -1):
        Rb = w[m - 1] + _suffix2(G * Rb)
        dG = dG + Rb * P[m - 1]
    return dG


def pair_grads(variant, sigma, x, y, w):
    """one pair: (d / dx, d / dy) of sum_m w[m - 1] k_m with respect to the POINTS x (Mp, D), y (Np, D); plain: x, y are the fp64 paths and
    the steps are their fp64 differences"""
    w = np.asarray(w, dtype=LD)
    if variant == "plain":
        dx, dy = np.diff(x, axis=0).astype(LD), np.diff(y, axis=0).astype(LD)
        dG = dG_of(dx @ dy.T, w)
        Tx, Ty = dG @ dy, dG.T @ dx
        gx, gy = np.zeros(x.shape, dtype=LD), np.zeros(y.shape, dtype=LD)
        gx[1:] += Tx
        gx[:-1] -= Tx
        gy[1:] += Ty
        gy[:-1] -= Ty
        return gx, gy
    dG = dG_of(lifted_G(x, y, sigma), w)
    H = np.zeros((x.shape[0], y.shape[0]), dtype=LD)      # the transposed second difference: d / d kap
    H[1:, 1:] += dG
    H[:-1, :-1] += dG
    H[1:, :-1] -= dG
    H[:-1, 1:] -= dG
    _, kap, _ = _lift_parts(x, y, sigma)
    e = x.astype(LD)[:, None, :] - y.astype(LD)[None, :, :]
    T = (H * kap * (LD(-2) / LD(sigma)))[:, :, None] * e
    return T.sum(1), -T.sum(0)


def want_grads(variant, sigma, X, Y, w, op):
    """-> (dX (A, Mp, D), dY or None) of sum_pairs sum_m w[m - 1, pair] k_m(pair) in long double; w (L, A, B), paired (L, P); op `sym`:
    Y is X and dX holds both arguments' parts.  X, Y: fp64 PATHS."""
    A, B = X.shape[0], Y.shape[0]
    gX, gY = np.zeros(X.shape, dtype=LD), np.zeros(Y.shape, dtype=LD)
    for a, b in _pairs(A, B, op == "paired"):
        gx, gy = pair_grads(variant, sigma, X[a], Y[b], w[:, a] if op == "paired" else w[:, a, b])
        gX[a] += gx
        (gX if op == "sym" else gY)[b] += gy
    return gX, (None if op == "sym" else gY)


def upstream_weights(scale, seed=1):
    """w[m - 1] = randn / max_pair scale[m] (the module docstring), 0 where that is no double -> (L,) + pairs fp64"""
    L = scale.shape[0] - 1
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((L,) + scale.shape[1:])
    for m in range(1, L + 1):
        top = float(np.max(scale[m]))
        w[m - 1] = w[m - 1] / top if np.isfinite(top) and top >= 1e-300 else 0.0
    return w


# ------------------------------------------------------------------------------------------------------------------- certificates
def _mp_of(v):
    """a long double as an mpmath number, exactly"""
    import mpmath
    m, e = np.frexp(LD(v))
    hi = np.float64(m)
    return mpmath.ldexp(mpmath.mpf(float(hi)) + mpmath.mpf(float(np.float64(m - LD(hi)))), int(e))


def mp_levels(variant, sigma, x, y, L, order):
    """the recursion of levels_of_G on one pair in mpmath at 50 digits, G by the DEFINITION (inner products of the steps; second
    differences of exp(-|x - y|^2 / sigma)) -> (k_0 .. k_L, scale_0 .. scale_L) as mpmath numbers"""
    import mpmath
    with mpmath.workdps(50):
        mp = mpmath.mpf
        xs, ys = [[mp(float(v)) for v in r] for r in x], [[mp(float(v)) for v in r] for r in y]
        if variant == "plain":
            G = [[mpmath.fsum(a * b for a, b in zip(r, c)) for c in ys] for r in xs]
        else:
            s = mp(float(sigma))
            K = [[mpmath.exp(-mpmath.fsum((a - b) ** 2 for a, b in zip(r, c)) / s) for c in ys] for r in xs]
            G = [[K[i + 1][j + 1] - K[i + 1][j] - K[i][j + 1] + K[i][j] for j in range(len(ys) - 1)] for i in range(len(xs) - 1)]
        M, N = len(G), len(G[0])
        zero = lambda: [[mp(0)] * N for _ in range(M)]

        def excl_rows(T):
            out = zero()
            for i in range(1, M):
                out[i] = [out[i - 1][j] + T[i - 1][j] for j in range(N)]
            return out

        def excl_cols(T):
            out = zero()
            for i in range(M):
                for j in range(1, N):
                    out[i][j] = out[i][j - 1] + T[i][j - 1]
            return out

        def add(S, T):
            return [[S[i][j] + T[i][j] for j in range(N)] for i in range(M)]

        def mul(T, f=1):
            return [[G[i][j] * T[i][j] / f for j in range(N)] for i in range(M)]
        R = [[G]]
        ks, mags = [mp(1)], [mp(1)]
        for m in range(1, L + 1):
            planes = [R[p][q] for p in range(len(R)) for q in range(len(R))]
            ks.append(mpmath.fsum(v for T in planes for r in T for v in r))
            mags.append(mpmath.fsum(abs(v) for T in planes for r in T for v in r))
            if m == L:
                break
            d, dn = len(R), min(m + 1, order)
            nxt = [[None] * dn for _ in range(dn)]
            for p in range(dn):
                for q in range(dn):
                    if p == 0 and q == 0:
                        nxt[0][0] = mul(excl_rows(excl_cols(functools.reduce(add, planes))))
                    elif p == 0:
                        nxt[0][q] = mul(excl_rows(functools.reduce(add, [R[pp][q - 1] for pp in range(d)])), q + 1)
                    elif q == 0:
                        nxt[p][0] = mul(excl_cols(functools.reduce(add, [R[p - 1][qq] for qq in range(d)])), p + 1)
                    else:
                        nxt[p][q] = mul(R[p - 1][q - 1], (p + 1) * (q + 1))
            R = nxt
        return ks, mags


def level_certificate(variant, sigma, x, y, L, order):
    """max over levels of |levels_of_G - mp_levels| / scale[m] on one pair (0 for a level whose scale is 0 on both sides)"""
    import mpmath
    ks, mags = levels_of_G(pair_G(variant, sigma, x, y), L, order)
    with mpmath.workdps(50):
        mk, mm = mp_levels(variant, sigma, x, y, L, order)
        worst = mpmath.mpf(0)
        for m in range(L + 1):
            d = abs(_mp_of(ks[m]) - mk[m])
            if mm[m] == 0:
                assert d == 0 and mags[m] == 0
                continue
            worst = max(worst, d / mm[m], abs(_mp_of(mags[m]) - mm[m]) / mm[m])
        return float(worst)


def fd_certificate(variant, sigma, x, y, w, points=((1, 0), (-1, -1), (0, 1))):
    """the gradient yardstick of one pair against central differences of the level yardstick in long double, h = 1e-6 of the path's
    coordinate scale -> max over the probed (point, coordinate) of both paths of |analytic - difference| / max |gradient of the path|"""
    gx, gy = pair_grads(variant, sigma, x, y, w)
    wl = np.asarray(w, dtype=LD)

    def loss(xv, yv):
        if variant == "plain":
            G = np.diff(xv, axis=0) @ np.diff(yv, axis=0).T
        else:
            G = lifted_G(xv, yv, sigma)
        return (wl * levels_of_G(G, len(wl), 1)[0][1:]).sum()
    worst = 0.0
    for side, g, P in (("x", gx, x), ("y", gy, y)):
        span = max(float(np.max(np.abs(np.diff(P, axis=0)))), 1e-300)
        h = LD(1e-6) * LD(span)
        for i, k in points:
            xp, xm, yp, ym = (t.astype(LD).copy() for t in (x, x, y, y))
            if side == "x":
                xp[i, k] += h
                xm[i, k] -= h
            else:
                yp[i, k] += h
                ym[i, k] -= h
            den = (xp[i, k] - xm[i, k]) if side == "x" else (yp[i, k] - ym[i, k])      # the step actually taken: exact in long double
            fd = (loss(xp, yp) - loss(xm, ym)) / den
            worst = max(worst, float(abs(fd - g[i, k]) / np.max(np.abs(g))))
    return worst


# ------------------------------------------------------------------------------------------------------------------- rows
# One row per launch-time mode of k_trunc_sig at the smallest shape that reaches it (upstream_gradients.TRUNC_MODES), L = 8 so that every
# unrolled level slot and every slab plane is read.  api: what the GPU test calls -- "object": TruncatedSigKernel on paths; "function":
# truncated_sig_kernel / truncated_sig_kernel_levels on STEPS; "long": HipBackend.truncated_long on steps (no_swap: the object's plain
# launch would serve these shapes on (Y, X)); claim: the instance that must be on the launch trace; route: (route op, order, D, M, N) of
# the sk_route_query that must say FUSED, M and N as that op counts them (steps; the points ops: points); invariant: families on which the
# kernel forms the quantity from differences, with the source that says so -- no allowance for the restatement's own loss there.
WHY_PLAIN = "truncated.py:655 (the object differences the paths; k_trunc_sig works on steps)"
WHY_POINTS = "sk_truncated.hip:268-272 (d2 from coordinate differences; first differences as kap_low expm1_nonpos(-|dX|))"


def _row(name, api, op, shape, variant="plain", order=1, f32=False, knobs=None, kw=None, claim=GENERAL, route=None, outputs=("levels", "weighted"),
         L=L_MAX):
    A, B, Mp, Np, D = shape
    steps = variant == "plain"
    inv = ("offset",) if steps else ("offset", "sigma>=1e2")
    return {"name": name, "api": api, "op": op, "shape": shape, "variant": variant, "order": order, "f32": f32, "knobs": knobs or {}, "kw": kw or {},
            "claim": claim, "route": route + (order, D, Mp - steps, Np - steps, L), "outputs": outputs, "L": L, "invariant": inv,
            "why": WHY_PLAIN if steps else WHY_POINTS, "id": "%s-%s-%s" % (name.replace(" ", "_"), op, "x".join(str(v) for v in shape))}


BASE, BASE_P, BASE_S = (3, 2, 20, 17, 3), (3, 3, 20, 17, 3), (3, 3, 20, 20, 3)
FORWARD = [
    _row("plain", "object", "gram", BASE, claim=ORDER1, route=("OP_TRUNCATED",)),
    _row("plain", "object", "paired", BASE_P, claim=ORDER1, route=("OP_TRUNCATED",)),
    _row("function weighted and normalized", "function", "gram", BASE, claim=ORDER1, route=("OP_TRUNCATED",), outputs=("weighted", "normalized")),
] + [_row("function levels order %d" % o, "function", "gram", BASE, order=o, route=("OP_TRUNCATED",)) for o in (2, 3, 4)] + [
    _row("plain dim 12", "object", "gram", (3, 2, 20, 17, 12), claim=ORDER1, route=("OP_TRUNCATED",)),      # (16 doubles per step, still <1, 2>)
    _row("plain fp32", "object", "gram", BASE, f32=True, claim=ORDER1, route=("OP_TRUNCATED",)),
    _row("points", "object", "gram", BASE, variant="rbf", route=("OP_TRUNCATED_RBF",)),
    _row("points", "object", "paired", BASE_P, variant="rbf", route=("OP_TRUNCATED_RBF",)),
    _row("points dim 12", "object", "gram", (3, 2, 20, 17, 12), variant="rbf", route=("OP_TRUNCATED_RBF",)),
    _row("points dim 12", "object", "paired", (3, 3, 20, 17, 12), variant="rbf", route=("OP_TRUNCATED_RBF",)),
    _row("long", "long", "gram", (3, 2, 130, 41, 3), knobs={"truncated_long": True}, route=("OP_TRUNCATED_LONG",)),
    _row("long dim 12", "long", "gram", (3, 2, 130, 41, 12), knobs={"truncated_long": True}, route=("OP_TRUNCATED_LONG",)),
]
_GRAD_MODES = [      # (name, variant, keywords, shape, claim, forward op, adjoint op)
    ("adjoint", "plain", {}, BASE, ORDER1, "OP_TRUNCATED", "OP_TRUNCATED_ADJOINT"),
    ("points adjoint", "rbf", {"points_adjoint": True}, BASE, GENERAL, "OP_TRUNCATED_RBF", "OP_TRUNCATED_RBF_ADJOINT"),
    ("long adjoint", "plain", {"long_adjoint": True}, (3, 2, 130, 41, 3), GENERAL, "OP_TRUNCATED_LONG", "OP_TRUNCATED_LONG_ADJOINT"),
    ("wide adjoint", "plain", {"wide_adjoint": True}, (3, 2, 20, 17, 9), GENERAL, "OP_TRUNCATED", "OP_TRUNCATED_WIDE_ADJOINT"),
]


def _grad_rows():
    rows = []
    for name, variant, kw, (A, B, Mp, Np, D), claim, fwd, adj in _GRAD_MODES:
        for op in ("gram", "paired", "sym"):
            shape = (A, A if op != "gram" else B, Mp, Mp if op == "sym" else Np, D)
            r = _row(name, "object", op, shape, variant=variant, kw=kw, claim=claim, route=(adj,), outputs=("dX",) if op == "sym" else ("dX", "dY"))
            r["forward_route"] = (fwd,) + r["route"][1:]
            rows.append(r)
    return rows


GRADIENT = _grad_rows()
ROWS = FORWARD + GRADIENT
ROW_BY_ID = {r["id"]: r for r in ROWS}
assert len(ROW_BY_ID) == len(ROWS)


def is_gradient(row):
    return "dX" in row["outputs"]


def is_invariant(row, fam, lab, st):
    return fam == "offset" or (row["variant"] == "rbf" and fam == "sigma" and st["sigma"] >= 1e2)


def cases(families=None):
    """[(row, family, parameter label, settings)] -- every cell of the GPU test"""
    out = []
    for row in ROWS:
        for fam, per in FAMILIES.items():
            if families is not None and fam not in families:
                continue
            for lab, st in per.get(row["variant"], []):
                if row["op"] == "sym" and (fam == "drift" or st.get("offset", (0, 0))[0] != st.get("offset", (0, 0))[1] or st.get("poison", "X")[0] == "Y"):
                    continue      # (one batch: nothing to drift away from, no separate shifts, no second batch to poison)
                out.append((row, fam, lab, st))
    return out


def case_id(c):
    row, fam, lab, st = c
    return "%s-%s-%s" % (row["id"], fam, lab.replace(" ", "_"))


def golden_key(row, fam, lab):
    return "%s|%s|%s" % (row["id"], fam, lab)


def golden_entries():
    return {golden_key(row, fam, lab): (row, fam, lab, st) for row, fam, lab, st in cases(MEASURED)}


def kernel_inputs(row, X, Y):
    """what the yardstick works on: a plain row's steps as torch forms them (the function and long rows are GIVEN these), an rbf row's points"""
    if row["variant"] == "plain":
        dX = steps_of(X, row["f32"])
        return dX, (dX if Y is X else steps_of(Y, row["f32"]))
    return X, Y


@functools.lru_cache(maxsize=None)
def _want(row_id, fam, lab, seed):
    row = ROW_BY_ID[row_id]
    st = dict(FAMILIES[fam][row["variant"]])[lab]
    X, Y = inputs(st, row, seed)
    kx, ky = kernel_inputs(row, X, Y)
    lev, scale = want_levels(row["variant"], st.get("sigma"), kx, ky, row["L"], row["order"], row["op"] == "paired")
    out = {"X": X, "Y": Y, "sigma": st.get("sigma"), "levels": lev, "scale": scale}
    if is_gradient(row):
        out["w"] = upstream_weights(scale)
        out["dX"], out["dY"] = want_grads(row["variant"], st.get("sigma"), X, Y, out["w"], row["op"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def case_want(row, fam, lab, seed=0):
    """inputs and the yardstick's results of a measured case, computed once per process and never written to"""
    return _want(row["id"], fam, lab, seed)


# ------------------------------------------------------------------------------------------------------------------- comparison
def n_nodes(row):
    A, B, Mp, Np, D = row["shape"]
    return Mp * Np


def level_floor(row, scale):
    """floor[m] = n_nodes 2^-1022 max(1, scale[m - 1]): what a result below the double range may be off by (a flush to zero passes,
    garbage does not); floor[0] = 0"""
    fl = np.zeros(scale.shape, dtype=LD)
    fl[1:] = n_nodes(row) * LD(TINY) * np.maximum(LD(1), scale[:-1])
    return fl


def level_errors(got, want, scale):
    """per level, max over pairs of |got - want| / scale[m][pair]; a pair whose scale is 0 must be met exactly (else inf); a non-finite
    result is inf -> (L + 1,) floats"""
    got = np.asarray(got, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = []
    for m in range(want.shape[0]):
        d, s = np.abs(got[m] - want[m]).ravel(), scale[m].ravel()
        d = np.where(np.isfinite(got[m].ravel().astype(np.float64)), d, LD(np.inf))
        e = np.where(s > 0, d / np.where(s > 0, s, 1), np.where(d == 0, LD(0), LD(np.inf)))
        out.append(float(np.max(e)))
    return np.array(out)


def grad_errors(got, want, skip_zero=False):
    """per path, max |got - want| / max |want| over the path -> (paths,); a path whose yardstick gradient is all zero must be met exactly
    (skip_zero: counts 0 -- the restatement is not under test)"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    n = want.shape[0]
    d = np.abs(got - want).reshape(n, -1).max(1)
    d = np.where(np.isfinite(got.reshape(n, -1).astype(np.float64)).all(1), d, LD(np.inf))
    top = np.abs(want).reshape(n, -1).max(1)
    return np.array([float(d[i] / top[i]) if top[i] > 0 else (0.0 if d[i] == 0 or skip_zero else np.inf) for i in range(n)])
