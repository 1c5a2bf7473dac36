"""SigKernel API and autograd surface, mirroring the reference's sigkernel/sigkernel.py:15-416.

Host code only: static kernels stay torch ops (rocBLAS under PyTorch-ROCm); increments, the
Goursat PDE solve and the adjoint PDE run in the HIP kernels of libsigkernel_amd.so through
:mod:`sigkernel_amd._lib`.  Differences from the reference that are not observable in results:

* the refined increment tensor of ``tile()`` (sigkernel.py:218, :364) is never built;
* the adjoint is solved lazily in ``backward`` for both Functions (the reference does it eagerly in
  ``_SigKernelGram.forward``, sigkernel.py:397-399) and contracted with the *analytic* derivative
  of the static kernel instead of the h = 1e-9 finite difference (sigkernel.py:313-341, :472-500);
* big batches are tiled by an HBM budget (``SigKernel.workspace_bytes``), not by ``max_batch``:
  results never depended on ``max_batch`` (sigkernel.py:31-39, :102-127) and still do not.
"""
import functools
from typing import NamedTuple

import torch

from . import _lib
from ._routes import routes
from .static_kernels import LinearKernel, RBFKernel

__all__ = ["SigKernel", "SigKernelStream", "_SigKernel", "_SigKernelGram", "k_kgrad", "pad_paths"]

_DEFAULT_WORKSPACE = 48 << 30  # bytes of transient HBM one call may use (288 GB part)


def _budget(device, requested):
    if requested is not None:
        return int(requested)
    if device.type == "cuda":
        free, _ = torch.cuda.mem_get_info(device)
        return int(min(_DEFAULT_WORKSPACE, 0.5 * free))
    return _DEFAULT_WORKSPACE


def _tiles(n_rows, bytes_per_row, budget):
    rows = int(max(1, min(n_rows, budget // max(1, bytes_per_row))))
    return [(a, min(a + rows, n_rows)) for a in range(0, n_rows, rows)]


def _cap_rows(bytes_per_row, pairs_per_row, budget):
    """bytes_per_row, raised where needed so that a row tile of `budget` bytes never holds more than _MAX_LAUNCH_PAIRS pairs."""
    return max(bytes_per_row, -(-int(budget) * int(pairs_per_row) // _MAX_LAUNCH_PAIRS))


class _Tile:
    """What forward keeps for the rows a0:a1 of a block: the terminal edges of their pairs (8 (MM + NN) bytes per pair; None where no
    kernel kept them) and, on the streaming route, the increments the static kernel formed for exactly these rows (else None)."""
    __slots__ = ("a0", "a1", "edges", "increments")

    def __init__(self, a0, a1, edges=None, increments=None):
        self.a0, self.a1, self.edges, self.increments = a0, a1, edges, increments

    def take_increments(self, dtype):
        """The kept increments where they are of `dtype`, else None.  The tile lets go of them either way: the caller's reference is
        the last one, so they are freed before the chain rule allocates."""
        inc, self.increments = self.increments, None
        return inc if inc is not None and inc.dtype == dtype else None


class _Kept:
    """The hand-off of one forward block to its backward: the row tiles with what each kept, and the forward values K of the block's
    pairs (what arms the fused adjoints' device-side rescue).  r0:r1 are the block's rows in the symmetric route's triangle.  The
    Functions hold it on `ctx` and take it off with _take: every decision about kept state is a method here."""
    __slots__ = ("tiles", "K", "r0", "r1")

    def __init__(self, r0=0, r1=None, K=None):
        self.tiles, self.K, self.r0, self.r1 = [], K, r0, r1

    def add(self, a0, a1, edges, increments=None):
        self.tiles.append(_Tile(a0, a1, edges, increments))

    def whole_edges(self, n_rows):
        """The edges where ONE tile kept them for all n_rows rows (what the fused forwards leave), else None."""
        t = self.tiles[0] if len(self.tiles) == 1 else None
        return t.edges if t is not None and (t.a0, t.a1) == (0, n_rows) else None

    def release(self):
        """Let go of every tile's edges and increments (K is the caller's output: it costs nothing to hold)."""
        self.tiles = []

    def row_tiles(self, n_rows, per_row, budget, strict=False):
        """Row tiles of a backward pass with what forward kept for them.  strict: never hand back a tile with more rows than `budget`
        allows (the kept tiling may have been sized for a route with less transient memory); a kept tiling that does not fit is
        released -- before the fresh tiles allocate -- and the adjoint sweeps forward itself."""
        tiles = [_Tile(a0, a1) for a0, a1 in _tiles(n_rows, per_row, budget)]
        full = self.whole_edges(n_rows)
        if full is not None:
            if len(tiles) == 1:
                return self.tiles
            self.tiles[0].increments = None     # (formed for all rows at once: of no use to a slice)
            per = full.numel() // n_rows       # the fused forward kept one block for all rows: slice it per tile
            return [_Tile(t.a0, t.a1, full[t.a0 * per:t.a1 * per]) for t in tiles]
        if self.tiles and (not strict or max(t.a1 - t.a0 for t in self.tiles) <= tiles[0].a1 - tiles[0].a0):
            return self.tiles                  # the tiling of forward, with the edges it kept (None where the strip kernels did not apply)
        self.release()
        return tiles


def _take(ctx, name="kept"):
    """The forward's hand-off, once: a second backward through a retained graph finds None and sweeps forward by itself."""
    kept = getattr(ctx, name, None)
    setattr(ctx, name, None)
    return kept


def _fused_static(static_kernel, gram):
    """(kind, param) when the static kernel is exactly one of the two the fused HIP kernels implement
    (sk_static_increments_*: static kernel + increments in one pass, G_static never materialised), else None.
    Subclasses and user-defined kernels always take the generic Gram_matrix / batch_kernel path."""
    if type(static_kernel) is LinearKernel:
        # the reference's Gram_matrix ignores `scale`, batch_kernel applies it to both arguments (static_kernels.py:24,33)
        return 0, (1.0 if gram else float(static_kernel.scale))
    if type(static_kernel) is RBFKernel:
        # (a tensor sigma is read as its value here; its gradient, where one is pending, is _static_params' business)
        sigma = static_kernel.sigma
        sigma = float(sigma.detach()) if isinstance(sigma, torch.Tensor) else float(sigma)
        if sigma > 0:
            return 1, sigma
    return None


def _static_params(static_kernel):
    """The static kernel's own tensors that require grad -- what SigKernel(exact_gradient=True) differentiates besides the paths:
    exactly RBFKernel: its ``sigma`` when that is a one-element tensor requiring grad; any static kernel that is a torch.nn.Module:
    its parameters that require grad; anything else: none."""
    if type(static_kernel) is RBFKernel:
        s = static_kernel.sigma
        return (s,) if isinstance(s, torch.Tensor) and s.numel() == 1 and s.requires_grad else ()
    if isinstance(static_kernel, torch.nn.Module):
        return tuple(p for p in static_kernel.parameters() if p.requires_grad)
    return ()


STREAM, FUSED, FUSED_MB, FUSED_MB_SWAP = _lib.ROUTE_STREAM, _lib.ROUTE_FUSED, _lib.ROUTE_FUSED_MB, _lib.ROUTE_FUSED_MB_SWAP
FUSED_SWAP = _lib.ROUTE_FUSED_SWAP
OP_FORWARD, OP_ADJOINT, OP_ADJOINT_SYM = _lib.OP_FORWARD, _lib.OP_ADJOINT, _lib.OP_ADJOINT_SYM


@functools.lru_cache(maxsize=4096)
def _route_query(route_fn, *key):
    """sk_route_query is a pure function of its arguments: one ctypes call (1.4 us) per distinct shape, a dictionary look-up after."""
    return route_fn(*key)


def _route(be, op, static_kernel, Xd, Yd, dyadic, naive, gram):
    """Which kernel family serves the call: the library's own answer (sk_route_query, csrc/sk_route.hip -- the one statement of the
    fused kernels' scope) for exactly LinearKernel / exactly RBFKernel, STREAM for every other static kernel; then the route
    switches (`sigkernel_amd.routes`: A/B measurements and the tests that compare a fused route with the streaming one)."""
    fused = _fused_static(static_kernel, gram)
    if fused is None or not hasattr(be, "route"):
        return STREAM
    if (fused[0] == 1 and routes.no_fused_rbf) or (op == OP_ADJOINT and routes.no_fused_adjoint):
        return STREAM
    # (a swapped ADJOINT -- second-argument sums of the one-band rbf adjoint on (y, x) -- exists for Gram calls only)
    no_swap = op == OP_ADJOINT and (not gram or routes.no_adjoint_swap or not hasattr(be, "second_argument_gradient"))
    r = _route_query(be.route, op, fused[0], Xd.shape[2], Xd.shape[1], Yd.shape[1], dyadic, bool(naive), Xd.element_size(), routes.no_stream, no_swap)
    if r in (FUSED_MB, FUSED_MB_SWAP) and routes.no_fused_mb:
        return STREAM
    return r


def _fused_forward(be, static_kernel, Xd, Yd, dyadic, naive, gram, keep_edges=False):
    """Whole forward in one kernel when sk_route_query says so (exactly LinearKernel / RBFKernel, dim <= 16, dyadic <= 2): the
    increments are formed inside the solver.  FUSED: sk_solve_fwd_linear_* / sk_solve_fwd_rbf_*; FUSED_MB (several bands per pair,
    wide paths): sk_solve_fwd_static_*.  None otherwise.  keep_edges (a gradient is pending): (K, edges) -- the edges of the family
    the ADJOINT route names, None when that adjoint forms its own (fp32 paths) or streams."""
    fused = _fused_static(static_kernel, gram)
    if fused is None or not hasattr(be, "route"):      # (the tests' oracle-backed back-end has no fused kernels: it streams)
        return None
    kind, param = fused
    Xd, Yd = Xd.contiguous(), Yd.contiguous()
    one_band = be.solve_fwd_fused_linear if kind == 0 else be.solve_fwd_fused_rbf
    f32 = Xd.dtype == torch.float32
    if keep_edges:
        ra = _route(be, OP_ADJOINT, static_kernel, Xd, Yd, dyadic, naive, gram)
        res = None
        if ra == FUSED and f32:
            # fp32 paths are staged and swept in fp64 whatever their dtype, and the one-band adjoint reads fp64 edges: the forward of
            # the up-cast paths gives the same values (rounded to fp32 below exactly as the fp32-output variant rounds them) AND the
            # edges, so that backward does not sweep forward a second time (Gram + backward 17.2 -> 13.5 ms at 512 x 512 pairs of C4's shape)
            res = one_band(Xd.double(), Yd.double(), param, dyadic, naive, gram, keep_edges=True)
            if res is not None:
                res = (res[0].to(Xd.dtype), res[1])
        elif ra == FUSED:
            res = one_band(Xd, Yd, param, dyadic, naive, gram, keep_edges=True)
        elif ra == FUSED_MB:
            res = be.solve_fwd_fused_static(kind, param, Xd, Yd, dyadic, naive, gram, keep_edges=True)
        elif ra == FUSED_SWAP and gram:
            # long first paths, short second ones: forward AND adjoint on (y, x) -- the edges are those of the pairs (b, a); fp32 paths
            # up-cast as for FUSED above
            res = one_band(Yd.double(), Xd.double(), param, dyadic, naive, True, keep_edges=True) if f32 else \
                one_band(Yd, Xd, param, dyadic, naive, True, keep_edges=True)
            if res is not None:
                res = (res[0].t().contiguous().to(Xd.dtype), res[1])
        if res is not None:
            return res
    rf = _route(be, OP_FORWARD, static_kernel, Xd, Yd, dyadic, naive, gram)
    res = None
    if rf == FUSED and keep_edges:
        # a streaming adjoint ahead: the one-band forward's strip edges are the layout sk_solve_adj_* reads (SK_FLAG_EDGES_GIVEN),
        # so that adjoint skips its own forward sweep
        res = one_band(Xd, Yd, param, dyadic, naive, gram, keep_edges=True)
        if res is not None:
            return res
    if rf not in (FUSED, FUSED_SWAP) and f32 and kind == 1 and dyadic == 0 and not keep_edges and not routes.no_fused_rbf:
        # the one-band RBF kernel at dyadic 0 is built for fp64 paths only: fp32 paths take it up-cast (they are staged in fp64 anyway)
        r8 = _route_query(be.route, OP_FORWARD, kind, Xd.shape[2], Xd.shape[1], Yd.shape[1], dyadic, bool(naive), 8, routes.no_stream)
        if r8 in (FUSED, FUSED_SWAP):
            res = one_band(Xd.double(), Yd.double(), param, dyadic, naive, gram) if r8 == FUSED else \
                one_band(Yd.double(), Xd.double(), param, dyadic, naive, gram)
            if res is not None:
                return (res.t().contiguous() if (r8 == FUSED_SWAP and gram) else res).to(Xd.dtype)
    if rf == FUSED:
        res = one_band(Xd, Yd, param, dyadic, naive, gram)
    elif rf == FUSED_SWAP:
        # long first paths, short second ones: k(y, x) through the one-band kernel (k and both static kernels are symmetric)
        res = one_band(Yd, Xd, param, dyadic, naive, gram)
        if res is not None and gram:
            res = res.t().contiguous()
    elif rf in (FUSED_MB, FUSED_MB_SWAP):
        res = be.solve_fwd_fused_static(kind, param, Xd, Yd, dyadic, naive, gram, swap=rf == FUSED_MB_SWAP)
    if res is None:
        return None
    return (res, None) if keep_edges else res


def _increments(be, static_kernel, Xd, Yd, gram, from_kernel=None):
    """Coarse increments of the static Gram for a tile: fused kernel when available, else the reference's route
    (static kernel in torch -> 4-corner difference, sigkernel.py:216-217 / :362-363).  from_kernel (a list): receives True when the
    fused static kernel formed them (what _tile_gradient's Linear / RBF branch would form again)."""
    fused = _fused_static(static_kernel, gram)
    if fused is not None and hasattr(be, "static_increments"):
        inc = be.static_increments(fused[0], fused[1], Xd.contiguous(), Yd.contiguous(), gram)
        if inc is not None:
            if from_kernel is not None:
                from_kernel.append(True)
            return inc
    G = (static_kernel.Gram_matrix(Xd, Yd) if gram else static_kernel.batch_kernel(Xd, Yd)).contiguous()
    return be.increments(G)


def _mb_pair_bytes(be, kind, Xd, Yd, dyadic):
    """Bytes per pair of what the multi-band fused routes hold in HBM: the edges sk_solve_fwd_static_* keeps (every band's bottom
    row and the terminal column), the adjoint's partial sums and its node-row-0 weights."""
    lay = be._adjoint_mb_layout(1, Xd.shape[1] - 1, Yd.shape[1] - 1, dyadic, Xd.shape[2], kind)
    if lay is None:
        return None
    _, rows, outw, edge_doubles, _, ncols = lay
    return 8 * (edge_doubles + rows * outw + ncols) + 64


def _upcast_tile(X, dyadic):
    return X.dtype == torch.float32 and dyadic == 2


def _tile_gradient(be, static_kernel, Xt, Yt, go, dyadic, naive, gram, kept=None):
    """dL/dX for one tile on the unfused routes: increments -> adjoint PDE (W = dK/d inc_c) -> chain through the static kernel.
    kept: the _Tile forward left for exactly these rows (its edges spare the adjoint's forward sweep, its increments the static kernel).

    Linear / RBF: sk_static_increments -> sk_solve_adj -> sk_static_adjoint.
    Generic (any duck-typed static kernel): G with autograd -> sk_increments -> sk_solve_adj ->
    sk_increments_adjoint (scaled by the upstream gradient) -> one vector-Jacobian product through the static kernel;
    this replaces the reference's h = 1e-9 finite difference (sigkernel.py:313-341, :472-500)."""
    fused = _fused_static(static_kernel, gram)
    edges = kept.edges if kept is not None else None
    if fused is not None and hasattr(be, "static_adjoint"):
        if _upcast_tile(Xt, dyadic) and edges is None:
            # fp32 paths at dyadic 2: the streaming adjoint exists for fp64 there.  The whole tile in fp64 -- increments formed
            # from the up-cast paths, adjoint, chain rule -- instead of fp32 increments up-cast in 4 GB chunks (round 2: 3x slower)
            g = _tile_gradient(be, static_kernel, Xt.double(), Yt.double(), go.double(), dyadic, naive, gram)
            return g.to(Xt.dtype)
        inc = kept.take_increments(Xt.dtype) if edges is not None else None      # (what _gram_block kept beside the edges)
        if inc is None:
            inc = be.static_increments(fused[0], fused[1], Xt, Yt, gram)
        if inc is not None:
            _, W = be.solve_adj(inc, dyadic, naive, edges=edges) if edges is not None else be.solve_adj(inc, dyadic, naive)
            del inc      # (freed before the chain rule allocates)
            return be.static_adjoint(fused[0], fused[1], Xt, Yt, W, go, gram)
    Xg = Xt.clone().requires_grad_(True)
    with torch.enable_grad():
        G = static_kernel.Gram_matrix(Xg, Yt) if gram else static_kernel.batch_kernel(Xg, Yt)
    inc = be.increments(G.detach().contiguous())
    _, W = be.solve_adj(inc, dyadic, naive, edges=edges) if edges is not None else be.solve_adj(inc, dyadic, naive)
    del inc
    dG = be.increments_adjoint(W, go)
    del W
    (g,) = torch.autograd.grad(G, Xg, dG)
    return g


def _fused_gradient(be, static_kernel, Xd, Yd, go, dyadic, naive, gram, kept, budget, route=FUSED):
    """dL/dX for all rows through the fused adjoints -- sk_linear_adjoint_fused_f64 / sk_rbf_adjoint_fused_f64 (route FUSED) or their
    multi-band forms (FUSED_MB): adjoint PDE and the static kernel's chain rule in one kernel, from the paths and the forward's
    edges; no matrix of size pairs x M x N -- one launch per row tile.  None when the kernel does not cover the case after all (the
    caller then takes the streaming route, tiled by ITS transient memory).  Exploding kernels are the library's business: with the
    forward values (kept.K, or what the forward re-run here returns) the launch takes such pairs out of the sweep and adds their
    exact, stored-grid share on the device (csrc/sk_adj_fused_rescue.hip) -- nothing is read back, a backward pass has no host
    synchronisation."""
    A, M = Xd.shape[0], Xd.shape[1]
    kind, param = _fused_static(static_kernel, gram)
    linear = kind == 0
    Kvals = kept.K
    if route == FUSED_MB:
        adj_mb = be.linear_adjoint_fused_mb if linear else be.rbf_adjoint_fused_mb
        # long / wide paths: sk_solve_fwd_static_* (edges) + the multi-band adjoint; per pair the edges, the partial sums and node row 0
        pair_bytes = _mb_pair_bytes(be, kind, Xd, Yd, dyadic)
        if pair_bytes is None:
            return None
        per_row = _cap_rows((Yd.shape[0] if gram else 1) * pair_bytes, Yd.shape[0] if gram else 1, budget)
        grad = torch.empty_like(Xd)
        for t in kept.row_tiles(A, per_row, budget, strict=True):
            a0, a1, edges = t.a0, t.a1, t.edges
            Xt = Xd[a0:a1].contiguous()
            Yt = Yd if gram else Yd[a0:a1].contiguous()
            got = go if go is None else go[a0:a1].reshape(-1).contiguous()
            Kt = None if Kvals is None else Kvals[a0:a1]
            res = adj_mb(Xt, Yt, param, dyadic, edges, got, gram=gram, kfinal=Kt, naive=naive) if edges is not None else None
            if res is None:    # no edges kept, or kept by another kernel in its own layout
                fw = be.solve_fwd_fused_static(kind, param, Xt, Yt, dyadic, naive, gram, keep_edges=True)
                edges = fw[1] if fw is not None else None
                if edges is None:
                    return None
                res = adj_mb(Xt, Yt, param, dyadic, edges, got, gram=gram, kfinal=fw[0], naive=naive)
                del edges
                if res is None:
                    return None
            grad[a0:a1] = res[0]
        return grad
    per_row = _cap_rows((64 * Yd.shape[0] + 2048 * M) if gram else 4096 * M, Yd.shape[0] if gram else 1, budget)      # edges and partial sums only
    grad = torch.empty_like(Xd)
    for t in kept.row_tiles(A, per_row, budget):
        a0, a1, edges = t.a0, t.a1, t.edges
        Xt = Xd[a0:a1].contiguous()
        Yt = Yd if gram else Yd[a0:a1].contiguous()
        Kt = None if Kvals is None else Kvals[a0:a1]
        if edges is None:     # (fp32 paths are swept in fp64: edges of the up-cast paths -- which is what their forward kept)
            fwd = be.solve_fwd_fused_linear if linear else be.solve_fwd_fused_rbf
            res = fwd(Xt.double(), Yt.double(), param, dyadic, naive, gram, keep_edges=True)
            edges = res[1] if res is not None else None
            Kt = res[0] if res is not None else None
        if edges is None:
            return None
        adj = be.linear_adjoint_fused if linear else be.rbf_adjoint_fused
        res = adj(Xt, Yt, param, dyadic, edges, None if go is None else go[a0:a1].reshape(-1).contiguous(), gram=gram, kfinal=Kt, naive=naive)
        if res is None:
            return None
        if a0 == 0 and a1 == A and res[0].shape == Xd.shape and res[0].dtype == Xd.dtype:
            return res[0]                # one tile: the kernel's own output, no copy
        grad[a0:a1] = res[0]
    return grad


def _swapped_gradient(be, static_kernel, Xd, Yd, go, dyadic, naive, kept, budget):
    """dL/dX of a Gram block whose FIRST paths are long and whose second paths fit the one-band adjoints' lanes (route FUSED_SWAP):
    the adjoint runs on the pairs (y_b, x_a) -- k and the static kernel are symmetric -- with the SECOND-argument sums of that sweep
    (sk_rbf_adjoint_fused_f64 / sk_linear_adjoint_fused_f64 with ypart), folded with the transposed upstream gradient:
    d k(x_a, y_b) / d x_a = d2 k(y_b, x_a).  Tiled over the rows of Y by the memory of the sums (48 / 64 bytes per pair and column).
    kept: the edges the forward kept for the swapped pairs (one block for all rows), else they are formed here.  None where the kernel declines (the caller streams)."""
    A, B = Xd.shape[0], Yd.shape[0]
    kind, param = _fused_static(static_kernel, True)
    linear = kind == 0
    fwd, adj = (be.solve_fwd_fused_linear, be.linear_adjoint_fused) if linear else (be.solve_fwd_fused_rbf, be.rbf_adjoint_fused)
    edges = kept.whole_edges(A)
    KT = None if kept.K is None else kept.K.double().t().contiguous()
    if edges is None:
        res = fwd(Yd, Xd, param, dyadic, naive, True, keep_edges=True)
        if res is None or res[1] is None:
            return None
        KT, edges = res
    per = edges.numel() // B
    goT = go.t().contiguous()                     # upstream gradient of the pair (b, a)
    grad = None
    for b0, b1 in _tiles(B, 64 * A * (Xd.shape[1] + 16), budget):
        res = adj(Yd[b0:b1].contiguous(), Xd, param, dyadic, edges[b0 * per:b1 * per], None, gram=True, yside=True,
                  kfinal=None if KT is None else KT[b0:b1], naive=naive, **({} if linear else {"yonly": True}))
        if res is None:
            return None
        g = be.second_argument_gradient(res[2], Xd, None if linear else param, goT[b0:b1], 0)
        grad = g if grad is None else grad + g
        del res
    return grad


def _rows_gradient(be, static_kernel, Xd, Yd, go, dyadic, naive, gram, kept, workspace_bytes):
    """dL/dX (A,M,D) of a Gram block (gram=True: go (A,B)) or a paired batch (go (A,)): the fused linear / RBF adjoint when it
    applies, else the unfused routes tiled over rows by their transient memory (3 (Linear/RBF) or 8 (generic) arrays of the
    size of the tile's increments).  kept: what forward left (_Kept), None where it left nothing or a backward has used it."""
    if kept is None:
        kept = _Kept()
    A, M, N = Xd.shape[0], Xd.shape[1], Yd.shape[1]
    budget = _budget(Xd.device, workspace_bytes)
    route = _route(be, OP_ADJOINT, static_kernel, Xd, Yd, dyadic, naive, gram)
    if route in (FUSED, FUSED_MB):
        g = _fused_gradient(be, static_kernel, Xd, Yd, go, dyadic, naive, gram, kept, budget, route)
        if g is not None:
            return g
    if route == FUSED_SWAP and gram:
        # (fp32 paths: swept in fp64 like every one-band call -- the edges their forward kept are those of the up-cast paths)
        g = _swapped_gradient(be, static_kernel, Xd.double(), Yd.double(), go.double(), dyadic, naive, kept, budget)
        if g is not None:
            return g.to(Xd.dtype)
        kept.release()    # (edges of the swapped pairs are of no use to the streaming route below)
    fused = _fused_static(static_kernel, gram) is not None
    esize = 8 if (fused and _upcast_tile(Xd, dyadic)) else Xd.element_size()
    per_row = (3 if fused else 8) * (Yd.shape[0] if gram else 1) * M * N * esize
    grad = torch.empty_like(Xd)
    for t in kept.row_tiles(A, per_row, budget, strict=True):
        a0, a1 = t.a0, t.a1
        grad[a0:a1] = _tile_gradient(be, static_kernel, Xd[a0:a1].contiguous(), Yd if gram else Yd[a0:a1].contiguous(),
                                     go[a0:a1].contiguous(), dyadic, naive, gram, t)
    return grad


def _functional(static_kernel):
    """Whether the static kernel is a kernel of function-valued paths (static_kernels.Linear_ID_Kernel, RBF_ID_Kernel, RBF_CEXP_Kernel,
    RBF_SQR_Kernel, or any kernel with the same two attributes): a ``features`` map (batch, T, ...) -> (batch, T, D_eff) and the
    ``base_kernel`` (Linear / RBF) that acts on the features."""
    return callable(getattr(static_kernel, "features", None)) and hasattr(static_kernel, "base_kernel")


class _FeatureMap:
    """The static kernel's feature map, applied once per distinct input tensor: where an input recurs (compute_Gram(X, X, sym=True)
    inside the loss wrappers) the same feature tensor comes back, so the symmetric routes and the doubled gradient still see one tensor."""

    def __init__(self, static_kernel):
        self.features = static_kernel.features
        self.seen = []

    def __call__(self, X):
        for t, f in self.seen:
            if t is X:
                return f
        f = self.features(X)
        self.seen.append((X, f))
        return f


def _check_inputs(X, Y, paired):
    if X.dim() != 3 or Y.dim() != 3:
        if X.dim() == 4 or Y.dim() == 4:
            raise ValueError("X and Y must have shape (batch, length, dim); paths of shape (batch, length, Lx, d) need a static kernel "
                             "of function-valued paths (Linear_ID_Kernel, RBF_ID_Kernel, RBF_CEXP_Kernel, RBF_SQR_Kernel) and go "
                             "through SigKernel's methods, which map them to features first")
        raise ValueError("X and Y must have shape (batch, length, dim)")
    if X.shape[2] != Y.shape[2]:
        raise ValueError("X and Y must have the same path dimension")
    if paired and X.shape[0] != Y.shape[0]:
        raise ValueError("compute_kernel needs the same batch size for X and Y")
    if X.dtype != Y.dtype or X.device != Y.device:
        raise ValueError("X and Y must share dtype and device")


class _SigKernel(torch.autograd.Function):
    """k_sig(x_i, y_i) for paired batches -- the reference's ``_SigKernel`` (sigkernel.py:201-343)."""

    @staticmethod
    def forward(ctx, X, Y, static_kernel, dyadic_order, _naive_solver=False, workspace_bytes=None):
        _check_inputs(X, Y, paired=True)
        be = _lib.get_backend()
        A, M, N = X.shape[0], X.shape[1], Y.shape[1]
        ctx.save_for_backward(X, Y)
        ctx.static_kernel, ctx.dyadic_order, ctx._naive_solver = static_kernel, dyadic_order, _naive_solver
        ctx.workspace_bytes = workspace_bytes
        if M < 2 or N < 2 or A == 0:  # a single point: the grid is its boundary, k = 1 (sigkernel.py:212-253 with MM = 0);
            return torch.ones(A, dtype=X.dtype, device=X.device)   # an empty batch: an empty result, like the CPU reference
        Xd, Yd = X.detach(), Y.detach()
        # (whether a gradient can be ASKED for -- not X.requires_grad: under torch.no_grad() a leaf X must not make the forward keep edges,
        # take the adjoint's kernel family or up-cast fp32 paths)
        need = bool(ctx.needs_input_grad[0])
        if need and hasattr(be, "solve_fwd_keep_edges"):
            # a gradient is pending: the forward keeps the terminal edges of every pair (8 (MM + NN) bytes each; a paired batch is
            # small), so that backward is ONE adjoint launch instead of a second forward sweep + the adjoint
            edge_bytes = 8.0 * A * (((M - 1) << dyadic_order) + ((N - 1) << dyadic_order) + 32)
            if _route(be, OP_ADJOINT, static_kernel, Xd, Yd, dyadic_order, _naive_solver, False) == FUSED_MB:
                pair_bytes = _mb_pair_bytes(be, _fused_static(static_kernel, False)[0], Xd, Yd, dyadic_order)
                edge_bytes = float(A) * (pair_bytes or 0)
            if edge_bytes <= _cost("keep_edges_fraction") * _budget(X.device, workspace_bytes):
                res = _fused_forward(be, static_kernel, Xd, Yd, dyadic_order, _naive_solver, gram=False, keep_edges=True)
                if res is not None:
                    K, edges = res
                    ctx.kept = _Kept(K=K.detach())
                    if edges is not None:
                        ctx.kept.add(0, A, edges)
                    return K
        K = _fused_forward(be, static_kernel, Xd, Yd, dyadic_order, _naive_solver, gram=False)
        if K is not None:
            ctx.kept = _Kept(K=K.detach()) if need else None     # forward values: what arms the fused adjoint's device-side rescue
            return K
        K = torch.empty(A, dtype=X.dtype, device=X.device)
        per_row = 2 * M * N * X.element_size()
        for a0, a1 in _tiles(A, per_row, _budget(X.device, workspace_bytes)):
            inc = _increments(be, static_kernel, Xd[a0:a1], Yd[a0:a1], gram=False)   # sigkernel.py:216-217 (:218 by index)
            K[a0:a1] = be.solve_fwd(inc, dyadic_order, _naive_solver)               # :231 / :246
        return K

    @staticmethod
    def backward(ctx, grad_output):
        X, Y = ctx.saved_tensors
        sk, d, naive = ctx.static_kernel, ctx.dyadic_order, ctx._naive_solver
        be = _lib.get_backend()
        A, M, N = X.shape[0], X.shape[1], Y.shape[1]
        if M >= 2 and N >= 2 and A > 0:
            go = grad_output.to(X.dtype).contiguous()
            grad_X = _rows_gradient(be, sk, X.detach().contiguous(), Y.detach().contiguous(), go, d, naive, False, _take(ctx),
                                    ctx.workspace_bytes)
        else:
            grad_X = torch.zeros_like(X)     # single points / an empty batch: k = 1 whatever X is
        return grad_X, None, None, None, None, None


# Cost rules (WHEN a route is the faster one -- not scope rules) live in ONE table, the library's (sk_cost_query, csrc/sk_route.hip: value +
# the A/B measurement behind it; tools/crossovers.py re-measures them).  None = the table's value; tests set an attribute to override.
_SYM_TILES = None              # "sym_tiles": row tiles of the symmetric shortcut: work = (T + 1) / (2 T) of the full Gram
_SYM_MIN_CELLS = None          # "sym_min_cells": below this the extra launches cost more than the saved solves
_SYM_MIN_ROWS = None           # "sym_min_rows": rows per block of the triangular adjoint
_SYM_STREAM_MIN_PATHS = None   # "sym_stream_min_paths": the streaming route's symmetric forward takes the blocked triangle from this many paths
_KEEP_EDGES_FRACTION = None    # "keep_edges_fraction": of the transient budget, what may stay allocated between forward and backward
_KEEP_INCREMENTS_FRACTION = None   # "keep_increments_fraction": ... and the streaming route's increments of a one-tile block beside them
_PAIRED_MERGE_CELLS = None     # "paired_merge_cells"
_MMD_STREAMS_MAX_PAIRS = None  # "mmd_streams_max_pairs"


def _cost(name):
    v = globals()["_" + name.upper()]
    return _lib.cost(name) if v is None else v


_MAX_LAUNCH_PAIRS = 1 << 30  # pairs per fused launch (the fused kernels index pairs with 32 bits and refuse 2^31 - 2^20 and more)


def _gram_block(be, static_kernel, Xd, Yd, dyadic_order, naive, workspace_bytes, rows_factor=None, keep=None):
    """K[a, b] for every pair of Xd x Yd (no autograd): fused kernel, or increments + solver tiled over rows of Xd.

    keep (a _Kept, when a gradient is pending): receives one tile per row tile -- the terminal row/column of every
    pair, 8(MM+NN) bytes per pair, which lets backward skip its forward sweep.  The reference keeps the whole solution
    grid for the same purpose (sigkernel.py:248, :397-399)."""
    A, B, M, N = Xd.shape[0], Yd.shape[0], Xd.shape[1], Yd.shape[1]
    if A * B > _MAX_LAUNCH_PAIRS and A > 1:
        # more pairs than one fused launch indexes (32 bits): row tiles of at most _MAX_LAUNCH_PAIRS pairs, each on its own route
        # (46400 x 46400 paths of 16 points, tools/experiments/r04_huge_batch.py: 2.8 s and 26 GB at the peak in three fused tiles against
        # 5.2 s and 114 GB streamed)
        rows = max(1, _MAX_LAUNCH_PAIRS // B)
        K = torch.empty(A, B, dtype=Xd.dtype, device=Xd.device)
        merged = []
        for a0 in range(0, A, rows):
            a1 = min(a0 + rows, A)
            sub = _Kept() if keep is not None else None
            K[a0:a1] = _gram_block(be, static_kernel, Xd[a0:a1], Yd, dyadic_order, naive, workspace_bytes, rows_factor, sub)
            if sub is not None:
                merged.extend(_Tile(a0 + t.a0, a0 + t.a1, t.edges, t.increments) for t in sub.tiles)
        # edges only when every tile kept them for all of its rows (else backward tiles by its own budget and sweeps forward itself)
        if merged and merged[0].a0 == 0 and merged[-1].a1 == A and all(s.a1 == t.a0 for s, t in zip(merged, merged[1:])):
            keep.tiles.extend(merged)
        return K
    budget = None   # (asked of the device only where it is needed: a small fused call does not pay for hipMemGetInfo)
    if keep is not None and hasattr(be, "solve_fwd_keep_edges"):
        budget = _budget(Xd.device, workspace_bytes)
        edge_bytes = 8.0 * A * B * (((M - 1) << dyadic_order) + ((N - 1) << dyadic_order) + 32)
        if _route(be, OP_ADJOINT, static_kernel, Xd, Yd, dyadic_order, naive, True) == FUSED_MB:
            # the multi-band forward keeps every band's bottom row: nb / 2 times the terminal row and column alone
            pair_bytes = _mb_pair_bytes(be, _fused_static(static_kernel, True)[0], Xd, Yd, dyadic_order)
            edge_bytes = float(A) * B * (pair_bytes or 0)
        if edge_bytes > _cost("keep_edges_fraction") * budget:
            keep = None
    else:
        keep = None
    if keep is not None:
        res = _fused_forward(be, static_kernel, Xd, Yd, dyadic_order, naive, gram=True, keep_edges=True)
        if res is not None:
            K, edges = res
            if edges is not None:
                keep.add(0, A, edges)      # one block for all rows: backward slices it per tile
            return K
    else:
        K = _fused_forward(be, static_kernel, Xd, Yd, dyadic_order, naive, gram=True)
        if K is not None:
            return K
    K = torch.empty(A, B, dtype=Xd.dtype, device=Xd.device)
    fused = _fused_static(static_kernel, True) is not None
    if budget is None:
        budget = _budget(Xd.device, workspace_bytes)
    # transient bytes per Gram row: G_static + inc_c on the generic route, inc_c alone on the fused one
    per_row = (rows_factor or (1 if fused else 2)) * B * M * N * Xd.element_size()
    tiles = _tiles(A, per_row, budget)
    for a0, a1 in tiles:
        by_kernel = []
        inc = _increments(be, static_kernel, Xd[a0:a1], Yd, True, by_kernel)     # sigkernel.py:362-363 (:364 by index)
        if keep is not None:
            K[a0:a1], edges = be.solve_fwd_keep_edges(inc, dyadic_order, naive)  # :378 / :395, + the edges for backward
            # one tile of moderate size: its increments are kept beside the edges, and backward does not evaluate the static
            # kernel a second time (a quarter of a gradient step on wide paths, profiles/r06_keep_inc.txt)
            keep_inc = edges is not None and by_kernel and len(tiles) == 1 and \
                inc.numel() * inc.element_size() <= _cost("keep_increments_fraction") * budget
            keep.add(a0, a1, edges, inc if keep_inc else None)
        else:
            K[a0:a1] = be.solve_fwd(inc, dyadic_order, naive)                    # :378 / :395
    return K


def _gram_symmetric(be, static_kernel, Xd, dyadic_order, naive, workspace_bytes, keep_blocks=None):
    """compute_Gram(X, X, sym=True): only the blocks on and above the diagonal of a T x T tiling are solved and
    mirrored, like the reference's CPU solver does pair by pair (cython_backend.pyx:74-97; its GPU path ignores `sym`).
    The result is exactly symmetric.  keep_blocks (a list, when a gradient is pending) receives one _Kept per
    row block r0:r1 for _SigKernelGram.backward's triangular adjoint (the caller gives each its rows of the finished K)."""
    A = Xd.shape[0]
    if keep_blocks is None and hasattr(be, "solve_fwd_fused_sym"):
        # exactly LinearKernel / RBFKernel within the single-band fused kernels' scope: the triangle in ONE launch, every value
        # written to both halves (sk_solve_fwd_linear_sym_* / sk_solve_fwd_rbf_sym_*)
        if _route(be, OP_FORWARD, static_kernel, Xd, Xd, dyadic_order, naive, True) == FUSED:
            kind, param = _fused_static(static_kernel, True)
            K = be.solve_fwd_fused_sym(kind, param, Xd, dyadic_order, naive)
            if K is not None:
                return K
    K = torch.empty(A, A, dtype=Xd.dtype, device=Xd.device)
    cells = float(A) * A * ((Xd.shape[1] - 1) << dyadic_order) ** 2
    # 8 block launches instead of 1: only worth it when the solve dwarfs the launches (measured: 128 x 128 pairs of
    # length 64 take 0.4 ms in one launch, 0.8 ms in blocks)
    tiles = int(_cost("sym_tiles"))
    T = tiles if (A >= 8 * tiles and cells >= _cost("sym_min_cells")) else 1
    if T == 1 and keep_blocks is None and A >= _cost("sym_stream_min_paths") and _SYM_MIN_CELLS is None and \
            _route(be, OP_FORWARD, static_kernel, Xd, Xd, dyadic_order, naive, True) == STREAM:
        # the streaming route (wide paths, dyadic >= 3, user-defined kernels): the static kernel and the increments are most of a pair's
        # cost, the blocked triangle pays from ~200 paths on whatever the grid (profiles/r06_sym_stream.txt)
        T = tiles
    if T > 1 and A >= 64 * T and keep_blocks is not None:
        T *= 2        # big batches with the fused adjoint: 16 row blocks solve 53 % of the square instead of 56 % (C4: -1 %)
    if keep_blocks is not None and T > 1:
        # with the adjoint in the blocks too, small blocks lose more to launches and pipeline fill than the triangle saves
        # (measured: 64 paths of length 700 in 8 blocks of 8 rows: backward 60 -> 74 ms): at least _SYM_MIN_ROWS rows each
        T = max(1, min(T, A // int(_cost("sym_min_rows"))))
    step = -(-A // T)
    for r0 in range(0, A, step):
        r1 = min(r0 + step, A)
        kept = _Kept(r0, r1) if keep_blocks is not None else None
        blk = _gram_block(be, static_kernel, Xd[r0:r1].contiguous(), Xd[r0:].contiguous(), dyadic_order, naive, workspace_bytes,
                          3 if keep_blocks is not None else None, kept)
        if keep_blocks is not None:
            keep_blocks.append(kept)
        K[r0:r1, r0:] = blk
        if r1 < A:
            K[r1:, r0:r1] = blk[:, r1 - r0:].t()
    # the diagonal blocks were solved in full: symmetrise them to the upper triangle too
    iu = torch.triu_indices(A, A, offset=1, device=Xd.device)
    K[iu[1], iu[0]] = K[iu[0], iu[1]]
    return K


def _keep_sym_values(sym_blocks, K):
    """Every row block of the triangle gets its rows of the finished K (r0:r1 against the columns from r0 on)."""
    Kd = K.detach()
    for blk in sym_blocks:
        blk.K = Kd[blk.r0:blk.r1, blk.r0:]


def _sym_triangle_ok(be, static_kernel, Xd, dyadic, naive):
    """Whether compute_Gram(X, X, sym=True) WITH a gradient solves the triangle only (a pair above the diagonal also stands for its
    mirror image, through the second-argument contraction of the same adjoint sweep), by the ADJOINT route of the shape:
      FUSED, RBFKernel, fp64   yes where sk_route_query(SK_OP_ADJOINT_SYM) says so -- sk_rbf_adjoint_fused_f64 with the second-argument sums
                               (_sym_fused_gradient; dim <= 4, 64 points at dyadic 1..2, 128 at dyadic 0); all pairs beyond
      FUSED, LinearKernel      no  -- the fused adjoint on ALL pairs is faster than any triangle route (14 vs 20 ms at the C3 shape)
      FUSED_MB                 no  -- likewise (C5's shape: 0.29 s on all pairs against 0.46 s on the streamed triangle)
      STREAM (fused static kernels beyond dim 16 / dyadic 2, or a route switch): yes where sk_static_adjoint2 exists (linear: dim <= 8)
    One predicate for the single-GPU Function and the sharded one (sigkernel_amd.distributed)."""
    fused = _fused_static(static_kernel, True)
    if fused is None or not hasattr(be, "static_adjoint2"):
        return False
    route = _route(be, OP_ADJOINT, static_kernel, Xd, Xd, dyadic, naive, True)
    if route == FUSED:      # (the library says where the second-argument sums exist and pay: sk_route_query(SK_OP_ADJOINT_SYM))
        return hasattr(be, "second_argument_gradient") and _route(be, OP_ADJOINT_SYM, static_kernel, Xd, Xd, dyadic, naive, True) == FUSED
    if route == STREAM:
        return Xd.shape[2] <= (8 if fused[0] == 0 else 32)
    return False


def _same_storage(Xd, Yd):
    return Xd.shape == Yd.shape and Xd.data_ptr() == Yd.data_ptr() and Xd.stride() == Yd.stride()


def _sym_fused_gradient(be, static_kernel, Xd, go, dyadic, naive, sym_blocks, budget):
    """dL/dX of compute_Gram(X, X, sym=True) from the triangular row blocks through the FUSED RBF adjoint with the
    second-argument sums (sk_rbf_adjoint_fused_f64 with ypart): per row block r0:r1 ONE launch over the solved pairs
    (a in r0:r1, b >= r0) gives the first-argument rows r0:r1 and, per pair, the sums that what the unsolved mirror pairs
    (b, a), b >= r1, owe to rows r1: is folded from (d1 K(x_b, x_a) = d2 K(x_a, x_b): the scheme is symmetric).  Neither the
    increments nor W exist in HBM, and exploding pairs are rescued on the device (each block's K: its rows of the forward's values).  None when
    the kernel does not cover the case or the forward kept no edges; the caller then takes the unfused triangular route."""
    if not (type(static_kernel) is RBFKernel and _route(be, OP_ADJOINT, static_kernel, Xd, Xd, dyadic, naive, True) == FUSED
            and Xd.dtype == torch.float64 and hasattr(be, "second_argument_gradient")):
        return None
    A, M = Xd.shape[0], Xd.shape[1]
    sigma = float(static_kernel.sigma)
    grad = torch.zeros_like(Xd)
    for blk in sym_blocks:
        r0, r1 = blk.r0, blk.r1
        edges = blk.whole_edges(r1 - r0)
        if edges is None:
            return None
        Xc = Xd[r0:].contiguous()
        nb = Xc.shape[0]
        # rows per launch by the memory of the second-argument sums (48 bytes per pair and node column)
        per_row = 64 * nb * (M + 16)
        per = edges.numel() // (r1 - r0)
        for a0, a1 in _tiles(r1 - r0, per_row, budget):
            Xt = Xd[r0 + a0:r0 + a1].contiguous()
            Kt = None if blk.K is None else blk.K[a0:a1]
            res = be.rbf_adjoint_fused(Xt, Xc, sigma, dyadic, edges[a0 * per:a1 * per], go[r0 + a0:r0 + a1, r0:].reshape(-1).contiguous(),
                                       gram=True, yside=r1 < A, kfinal=Kt, naive=naive)
            if res is None:
                return None
            grad[r0 + a0:r0 + a1] += res[0]
            if r1 < A:   # upstream gradient of the mirror pair (b, a) is go[b, a]
                grad[r1:] += be.second_argument_gradient(res[2], Xc, sigma, go[r0:, r0 + a0:r0 + a1].t(), r1 - r0)
            del res
    return grad


def _sym_unfused_gradient(be, kind, param, Xd, go, dyadic, naive, sym_blocks, budget):
    """The same through sk_static_increments -> sk_solve_adj -> sk_static_adjoint (first argument) + sk_static_adjoint2 (second
    argument of the SAME W, weighted by the transposed upstream gradient); owns the stored-grid rescue."""
    A, M, N = Xd.shape[0], Xd.shape[1], Xd.shape[1]
    if _upcast_tile(Xd, dyadic) and all(t.edges is None for blk in sym_blocks for t in blk.tiles):
        # fp32 paths at dyadic 2 without kept edges: the whole route in fp64 (see _tile_gradient)
        return _sym_unfused_gradient(be, kind, param, Xd.double(), go.double(), dyadic, naive, sym_blocks, budget).to(Xd.dtype)
    grad_X = torch.zeros_like(Xd)
    for blk in sym_blocks:
        r0, r1 = blk.r0, blk.r1
        Xr, Xc = Xd[r0:r1].contiguous(), Xd[r0:].contiguous()
        go_blk = go[r0:r1, r0:].contiguous()
        go_t = go[r0:, r0:r1].t().contiguous()         # [a, b] -> upstream gradient of the mirror pair (b, a)
        per_row = 3 * Xc.shape[0] * M * N * Xd.element_size()
        for t in blk.row_tiles(r1 - r0, per_row, budget):
            a0, a1, edges = t.a0, t.a1, t.edges
            Xt = Xr[a0:a1].contiguous()
            inc = t.take_increments(Xt.dtype) if edges is not None else None      # (what _gram_block kept beside the edges)
            if inc is None:
                inc = be.static_increments(kind, param, Xt, Xc, True)
            _, W = be.solve_adj(inc, dyadic, naive, edges=edges) if edges is not None else be.solve_adj(inc, dyadic, naive)
            del inc
            grad_X[r0 + a0:r0 + a1] += be.static_adjoint(kind, param, Xt, Xc, W, go_blk[a0:a1].contiguous(), True)
            if r1 < A:
                g2 = be.static_adjoint2(kind, param, Xt, Xc, W, go_t[a0:a1].contiguous(), r1 - r0)
                if g2 is None:      # (_sym_triangle_ok keeps such shapes off the triangle: a caller that bypassed it)
                    raise RuntimeError("sigkernel_amd: the triangular adjoint has no second-argument kernel for path dim %d" % Xd.shape[2])
                grad_X[r1:] += g2
            del W
    return grad_X


class _SigKernelGram(torch.autograd.Function):
    """Gram matrix k_sig(x_i, y_j) -- the reference's ``_SigKernelGram`` (sigkernel.py:347-416)."""

    @staticmethod
    def forward(ctx, X, Y, static_kernel, dyadic_order, sym=False, _naive_solver=False, workspace_bytes=None):
        _check_inputs(X, Y, paired=False)
        be = _lib.get_backend()
        A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
        ctx.save_for_backward(X, Y)
        ctx.static_kernel, ctx.dyadic_order, ctx._naive_solver = static_kernel, dyadic_order, _naive_solver
        ctx.workspace_bytes = workspace_bytes
        ctx.sym_blocks = ctx.kept = None
        if M < 2 or N < 2 or A == 0 or B == 0:   # single points: k = 1; an empty batch: an empty matrix
            return torch.ones(A, B, dtype=X.dtype, device=X.device)
        Xd, Yd = X.detach(), Y.detach()
        need, need_y = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])      # (not need: see _SigKernel.forward)
        # `sym`: the reference's GPU path ignores it (sigkernel.py:366-382) and its CPU path silently assumes X is Y.
        # Here it halves the work when that assumption can be checked (same storage) and no gradient is needed.
        if sym and _same_storage(Xd, Yd):
            if not need and not need_y:
                return _gram_symmetric(be, static_kernel, Xd.contiguous(), dyadic_order, _naive_solver, workspace_bytes)
            # with a gradient: the triangular forward AND a triangular adjoint (a pair above the diagonal also stands for
            # its mirror image, through the second-argument contraction of the same W) -- fused static kernels only
            # (the fused linear adjoint is faster on all pairs than the unfused one on the triangle: 14 vs 20 ms at the C3 shape)
            # (long / wide RBF paths: the multi-band fused adjoint on ALL pairs beats the unfused triangle -- C5's shape 0.29 s against 0.46 s)
            if need and need_y and _sym_triangle_ok(be, static_kernel, Xd, dyadic_order, _naive_solver):
                ctx.sym_blocks = []
                K = _gram_symmetric(be, static_kernel, Xd.contiguous(), dyadic_order, _naive_solver, workspace_bytes,
                                    ctx.sym_blocks)
                _keep_sym_values(ctx.sym_blocks, K)
                return K
        fused = _fused_static(static_kernel, True) is not None
        # with a gradient pending, tile like backward will, so that the caching allocator can reuse the same blocks
        rows_factor = (3 if fused else 8) if need else None
        ctx.kept = _Kept() if need else None
        K = _gram_block(be, static_kernel, Xd, Yd, dyadic_order, _naive_solver, workspace_bytes, rows_factor, ctx.kept)
        if sym and _same_storage(Xd, Yd):   # all pairs were solved (fused adjoint ahead): still hand back an exactly symmetric matrix
            iu = torch.triu_indices(A, A, offset=1, device=K.device)
            K[iu[1], iu[0]] = K[iu[0], iu[1]]
        if need:
            ctx.kept.K = K.detach()     # forward values: what arms the fused adjoints' device-side rescue
        return K

    @staticmethod
    def backward(ctx, grad_output):
        X, Y = ctx.saved_tensors
        sk, d, naive = ctx.static_kernel, ctx.dyadic_order, ctx._naive_solver
        be = _lib.get_backend()
        A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
        grad_X = None
        sym_blocks = _take(ctx, "sym_blocks")
        if M >= 2 and N >= 2 and sym_blocks:
            # compute_Gram(X, X, sym=True): per row block r0:r1 the pairs (a, b >= r0) were solved.  Their first-argument
            # contraction gives rows r0:r1; the second-argument contraction of the SAME W, weighted by the transposed
            # upstream gradient, gives what the unsolved mirror pairs (b, a), b >= r1, owe to rows r1: (K is symmetric, so
            # d1 K(x_b, x_a) = d2 K(x_a, x_b)).  The reference's 2x rule (sigkernel.py:410-412) is applied below as usual.
            Xd = X.detach().contiguous()
            go = grad_output.to(X.dtype).contiguous()
            kind, param = _fused_static(sk, True)
            budget = _budget(X.device, ctx.workspace_bytes)
            g_fused = _sym_fused_gradient(be, sk, Xd, go, d, naive, sym_blocks, budget)
            if g_fused is not None:
                grad_X = g_fused
            else:
                grad_X = _sym_unfused_gradient(be, kind, param, Xd, go, d, naive, sym_blocks, budget)
        elif M >= 2 and N >= 2 and A > 0 and B > 0:
            go = grad_output.to(X.dtype).contiguous()
            grad_X = _rows_gradient(be, sk, X.detach().contiguous(), Y.detach().contiguous(), go, d, naive, True, _take(ctx),
                                    ctx.workspace_bytes)
        # the reference doubles the gradient when Y requires grad (written for compute_Gram(X, X) with a
        # symmetric grad_output, sigkernel.py:410-412) and never returns a gradient for Y
        if grad_X is None:
            grad_X = torch.zeros_like(X)     # single points / an empty batch: k = 1 whatever X is
        elif ctx.needs_input_grad[1]:
            grad_X = 2 * grad_X
        return grad_X, None, None, None, None, None, None


def _exact_static_route(be, static_kernel, gram, dim, params):
    """How _exact_tile runs the chain rule through the static kernel: "fused" (sk_static_adjoint_* / sk_static_adjoint2_*), "param" (the
    same with dL/dsigma from k_static_rbf_adj's parameter mode: RBFKernel.sigma pending, a backend with static_adjoint_param, at most
    its MAX_FUSED_DIM dims) or "generic" (the static kernel in torch and one vector-Jacobian product)."""
    fused = _fused_static(static_kernel, gram)
    if fused is None or not hasattr(be, "static_adjoint"):
        return "generic"
    if not params:
        return "fused"
    if fused[0] == 1 and hasattr(be, "static_adjoint_param") and dim <= getattr(be, "MAX_FUSED_DIM", 0):
        return "param"
    return "generic"


def _exact_tile(be, static_kernel, Xt, Yt, go, dyadic, naive, gram, need_x, need_y, cells=None, sources=None, params=()):
    """(dL/dX, dL/dY, [dL/dparam ...]) of one tile under exact_gradient=True (None where not needed): increments -> sk_solve_adj_* with SK_FLAG_DISCRETE
    (W = the exact derivative of the solver's value with respect to every coarse increment) -> the chain rule through the static
    kernel for BOTH arguments, from the same W.

    Linear / RBF: sk_static_adjoint for X; for Y sk_static_adjoint2 (Gram) or, where that has no kernel (paired batches, linear paths
    wider than 8 dims), sk_static_adjoint on the swapped pairs with W transposed (both static kernels are symmetric).
    Generic (any duck-typed static kernel): sk_increments_adjoint + ONE vector-Jacobian product through the static kernel for both.

    cells (ragged batches): (cx, cy), int32 coarse cells (length - 1) of the tile's paths on either side.  The pairs' table -- row
    (cx[a], cy[b]) for pair a * B + b of a Gram tile, (cx[p], cy[p]) paired -- goes with the launch (SK_FLAG_RAGGED): every pair is
    swept on its own sub-grid and W is exactly zero elsewhere, so the chain rule below runs unchanged on the padded paths and gives
    the padding an exactly zero gradient.

    sources (prefix calls, in place of go: pass go=None): S (a, B, M - 1, N - 1) for a Gram tile, (a, M - 1, N - 1) paired -- dL/d(prefix
    kernel) of every coarse node (m, n), m, n >= 1, of every pair.  They go with the launch (SK_FLAG_SOURCES): W is then dL/d(increments)
    itself, and the chain rule below runs with a unit upstream weight.

    params (_static_params: the static kernel's tensors with a gradient pending): their gradients come back as the third result, one
    fp64 tensor each.  RBFKernel.sigma up to 32 dims: ONE k_static_rbf_adj launch in its parameter mode gives dL/dX and dL/dsigma
    (be.static_adjoint_param), whether or not X needs its gradient.  Every other case -- RBF beyond 32 dims, torch.nn.Module kernels, a
    backend without that method -- is the generic branch with the parameters among the inputs of its one vector-Jacobian product; a
    parameter the static kernel does not use gets zeros."""
    more = {}
    if sources is not None:
        more["sources"] = sources
        go = torch.ones(sources.shape[:-2], dtype=sources.dtype, device=sources.device)
    if cells is not None:
        cx, cy = cells
        if gram:
            more["cells"] = torch.stack((cx[:, None].expand(-1, cy.shape[0]), cy[None, :].expand(cx.shape[0], -1)), dim=-1).contiguous()
        else:
            more["cells"] = torch.stack((cx, cy), dim=-1).contiguous()
    fused = _fused_static(static_kernel, gram)
    inc = None
    route = _exact_static_route(be, static_kernel, gram, Xt.shape[2], params)
    one_launch = route == "param"
    if route != "generic":
        inc = be.static_increments(fused[0], fused[1], Xt, Yt, gram)
    if inc is not None:
        kind, param = fused
        _, W = be.solve_adj(inc, dyadic, naive, discrete=True, **more)
        del inc
        gp = []
        if one_launch:
            gx, dparam = be.static_adjoint_param(kind, param, Xt, Yt, W, go, gram)
            gp = [dparam]
            if not need_x:
                gx = None
        else:
            gx = be.static_adjoint(kind, param, Xt, Yt, W, go, gram) if need_x else None
        gy = None
        if need_y:
            if gram and hasattr(be, "static_adjoint2"):
                gy = be.static_adjoint2(kind, param, Xt, Yt, W, go, 0)
            if gy is None:
                Wt = (W.transpose(0, 1) if gram else W).transpose(-1, -2).contiguous()     # the pair (b, a), cells (j, i)
                gy = be.static_adjoint(kind, param, Yt, Xt, Wt, go.t().contiguous() if gram else go, gram)
        return gx, gy, gp
    Xg, Yg = Xt.clone().requires_grad_(need_x), Yt.clone().requires_grad_(need_y)
    with torch.enable_grad():
        G = static_kernel.Gram_matrix(Xg, Yg) if gram else static_kernel.batch_kernel(Xg, Yg)
    _, W = be.solve_adj(be.increments(G.detach().contiguous()), dyadic, naive, discrete=True, **more)
    dG = be.increments_adjoint(W, go)
    del W
    wrt = [t for t, need in ((Xg, need_x), (Yg, need_y)) if need] + list(params)
    grads = list(torch.autograd.grad(G, wrt, dG, allow_unused=True))
    gx = (grads.pop(0) if need_x else None)
    gy = (grads.pop(0) if need_y else None)
    gp = [torch.zeros(p.shape, dtype=torch.float64, device=Xt.device) if g is None else g.detach().to(device=Xt.device, dtype=torch.float64)
          for p, g in zip(params, grads)]
    return (torch.zeros_like(Xt) if need_x and gx is None else gx), (torch.zeros_like(Yt) if need_y and gy is None else gy), gp


def _exact_gradient(be, static_kernel, Xd, Yd, go, dyadic, naive, gram, workspace_bytes, need_x, need_y, cells=None, sources=None,
                    params=()):
    """(dL/dX, dL/dY, [dL/dparam ...]) of a Gram block (go (A, B)) or a paired batch (go (A,)) under exact_gradient=True, over row tiles sized like
    _rows_gradient's streaming tiles, with the stored-grid scratch of the discrete adjoint (min(pairs, 1024) slots of two fine grids,
    at most _lib.HipBackend.GRID_SCRATCH_BYTES) taken out of the budget first -- though never more than half of it.  fp32 paths are
    up-cast: the whole backward runs in fp64 and the gradients are rounded to fp32 at the end.  cells (ragged batches): (cx (A,), cy),
    int32 coarse cells of every path, length - 1; each row tile takes its slice (_exact_tile).  sources (prefix calls, in place of go:
    pass go=None): a function (a0, a1) -> the sources of rows a0..a1 in the paths' dtype (_exact_tile), built tile by tile so that nothing
    of size pairs x M x N outlives a tile; the tiles are those of a call with go.  params (_static_params): the static kernel's tensors
    with a gradient pending; their gradients are the third result, one fp64 tensor of the parameter's element count on the paths' device
    each (_exact_tile), summed over the row tiles in tile order."""
    if Xd.dtype != torch.float64:
        up = None if sources is None else (lambda a0, a1: sources(a0, a1).double())
        gx, gy, gp = _exact_gradient(be, static_kernel, Xd.double(), Yd.double(), None if go is None else go.double(), dyadic, naive, gram,
                                     workspace_bytes, need_x, need_y, cells, up, params)
        return (None if gx is None else gx.to(Xd.dtype)), (None if gy is None else gy.to(Yd.dtype)), gp
    A, M, N = Xd.shape[0], Xd.shape[1], Yd.shape[1]
    Bp = Yd.shape[0] if gram else 1
    budget = _budget(Xd.device, workspace_bytes)
    slot = 16 * (((M - 1) << dyadic) + 1) * (((N - 1) << dyadic) + 1)
    scratch = min(min(1024, A * Bp) * slot, getattr(be, "GRID_SCRATCH_BYTES", 2 << 30))
    fused = _exact_static_route(be, static_kernel, gram, Xd.shape[2], params) != "generic"
    per_row = (3 if fused else 8) * Bp * M * N * Xd.element_size()
    gx = torch.empty_like(Xd) if need_x else None
    gy = torch.zeros_like(Yd) if (need_y and gram) else (torch.empty_like(Yd) if need_y else None)
    gp = None
    for a0, a1 in _tiles(A, per_row, max(budget - scratch, budget // 2)):
        tx, ty, tp = _exact_tile(be, static_kernel, Xd[a0:a1].contiguous(), Yd if gram else Yd[a0:a1].contiguous(),
                                 None if go is None else go[a0:a1].contiguous(), dyadic, naive, gram, need_x, need_y,
                                 None if cells is None else (cells[0][a0:a1], cells[1] if gram else cells[1][a0:a1]),
                                 None if sources is None else sources(a0, a1).contiguous(), params)
        gp = tp if gp is None else [g + t for g, t in zip(gp, tp)]
        if need_x:
            gx[a0:a1] = tx
        if need_y and gram:
            gy += ty            # every row tile meets every path of Y
        elif need_y:
            gy[a0:a1] = ty
    return gx, gy, gp


def _param_grads(params, gp, needs):
    """The backward results of the trailing parameter inputs: every gradient in its parameter's shape, dtype and device (gp: what
    _exact_gradient returned, or None -- one-point paths and empty batches: k = 1 whatever the parameters are)"""
    return tuple(None if not need else torch.zeros_like(p) if gp is None else g.reshape(p.shape).to(device=p.device, dtype=p.dtype)
                 for p, g, need in zip(params, gp if gp is not None else params, needs))


class _SigKernelExact(torch.autograd.Function):
    """compute_kernel / compute_Gram under SigKernel(exact_gradient=True): the values of _SigKernel / _SigKernelGram on whatever route
    they take without a gradient pending (nothing is kept for backward), and in backward the TRUE gradient of those values -- the
    adjoint of the discrete solver (sk_solve_adj_* with SK_FLAG_DISCRETE), for both arguments.  No 2x rule: when X is Y, autograd adds
    the two contributions."""

    @staticmethod
    def forward(ctx, X, Y, static_kernel, dyadic_order, gram, sym, _naive_solver, workspace_bytes, *params):
        ctx.save_for_backward(X, Y, *params)
        ctx.args = (static_kernel, dyadic_order, gram, _naive_solver, workspace_bytes)
        if gram:
            return _SigKernelGram.forward(_NoGradCtx(), X, Y, static_kernel, dyadic_order, sym, _naive_solver, workspace_bytes)
        return _SigKernel.forward(_NoGradCtx(), X, Y, static_kernel, dyadic_order, _naive_solver, workspace_bytes)

    @staticmethod
    def backward(ctx, grad_output):
        X, Y, *params = ctx.saved_tensors
        static_kernel, d, gram, naive, workspace_bytes = ctx.args
        need_x, need_y = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        gp = None
        if X.shape[1] < 2 or Y.shape[1] < 2 or X.shape[0] == 0 or Y.shape[0] == 0:   # single points / empty batches: k = 1 whatever the paths
            gx, gy = (torch.zeros_like(X) if need_x else None), (torch.zeros_like(Y) if need_y else None)
        else:
            gx, gy, gp = _exact_gradient(_lib.get_backend(), static_kernel, X.detach().contiguous(), Y.detach().contiguous(),
                                         grad_output.to(X.dtype).contiguous(), d, naive, gram, workspace_bytes, need_x, need_y,
                                         params=params)
        return (gx, gy, None, None, None, None, None, None) + _param_grads(params, gp, ctx.needs_input_grad[8:])


class _SigKernelRaggedExact(torch.autograd.Function):
    """compute_kernel_ragged / compute_Gram_ragged under SigKernel(exact_gradient=True): forward is _prefix_at -- the values of the
    no-grad call, bit for bit -- and backward the true gradient of those values for both arguments: the exact adjoint of the discrete
    solver run on every pair's own sub-grid (sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_RAGGED), then _exact_gradient's chain rule
    on the paths with every padded point overwritten by its path's last true point (_repeat_last_point).  The padding receives exactly
    zero whatever it holds -- huge values, NaN and inf included -- and never reaches a true point's gradient
    (tests/test_gpu_prefix_value_regimes.py)."""

    @staticmethod
    def forward(ctx, X, Y, lx, ly, static_kernel, dyadic_order, gram, _naive_solver, workspace_bytes, *params):
        ctx.save_for_backward(X, Y, lx, ly, *params)
        ctx.args = (static_kernel, dyadic_order, gram, _naive_solver, workspace_bytes)
        return _prefix_at(_lib.get_backend(), static_kernel, X.detach(), Y.detach(), lx, ly, dyadic_order, _naive_solver, gram,
                          workspace_bytes)

    @staticmethod
    def backward(ctx, grad_output):
        X, Y, lx, ly, *params = ctx.saved_tensors
        static_kernel, d, gram, naive, workspace_bytes = ctx.args
        need_x, need_y = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        gp = None
        if X.shape[1] < 2 or Y.shape[1] < 2 or X.shape[0] == 0 or Y.shape[0] == 0:   # single points / empty batches: k = 1 whatever the paths
            gx, gy = (torch.zeros_like(X) if need_x else None), (torch.zeros_like(Y) if need_y else None)
        else:
            # W is exactly zero outside a pair's sub-grid, but the static stage still evaluates |x|^2 + |y|^2 - 2 <x, y> and x - y on the
            # padding: 0 * (inf - inf) for a padding whose squares or differences overflow, or that is not finite.  So the chain rule
            # runs on the paths padded with their last TRUE point: every true-point sum gains +-0 from the padding, the padding's own
            # gradient is 0 * finite, and a batch of full lengths is handed on as it is.
            gx, gy, gp = _exact_gradient(_lib.get_backend(), static_kernel, _repeat_last_point(X.detach(), lx).contiguous(),
                                         _repeat_last_point(Y.detach(), ly).contiguous(),
                                         grad_output.to(X.dtype).contiguous(), d, naive, gram, workspace_bytes, need_x, need_y,
                                         (lx - 1, ly - 1), params=params)
        return (gx, gy, None, None, None, None, None, None, None) + _param_grads(params, gp, ctx.needs_input_grad[9:])


def _prefix_sources(go, nodes, Mc, Nc):
    """grad_output of a prefix call (rows of a tile: (a, B, ...) Gram, (a, ...) paired; `...` = (M, N) for nodes="all", else the slice's
    length) -> the sources (..., Mc, Nc) of the adjoint sweep: the weight of every coarse node (m, n) with m, n >= 1.  Row 0 and column
    0 of a prefix grid are the constant 1 and element 0 of every slice with them: their weights reach no path."""
    if nodes == "all":
        return go[..., 1:, 1:]
    S = torch.zeros(go.shape[:-1] + (Mc, Nc), dtype=go.dtype, device=go.device)
    if nodes == "diagonal":
        torch.diagonal(S, dim1=-2, dim2=-1).copy_(go[..., 1:])
    elif nodes == "last_row":
        S[..., Mc - 1, :] = go[..., 1:]
    else:
        S[..., :, Nc - 1] = go[..., 1:]
    return S


class _SigKernelPrefixExact(torch.autograd.Function):
    """compute_Gram_prefixes / compute_kernel_prefixes (every `nodes` mode) under SigKernel(exact_gradient=True): forward is _prefix_grid
    -- the values of the no-grad call, bit for bit, on whatever route it takes -- and backward the true gradient of sum(grad_output *
    values) for both arguments.  The discrete solver is a linear recursion in K, so the adjoint of ANY weighted sum of coarse nodes is
    one reverse sweep per pair with each weight injected at its own node (sk_solve_adj_* with SK_FLAG_DISCRETE | SK_FLAG_SOURCES): a
    backward costs what compute_Gram's does under exact_gradient=True, however many nodes carry a weight.  W is then dL/d(increments)
    and _exact_gradient's chain rule runs with a unit upstream weight.  nodes="diagonal" on paths of unequal length touches the first
    T = min(len_x, len_y) points of either side alone: the backward runs on the truncated paths and the points cut away get exactly
    zero."""

    @staticmethod
    def forward(ctx, X, Y, static_kernel, dyadic_order, gram, nodes, _naive_solver, workspace_bytes, *params):
        ctx.save_for_backward(X, Y, *params)
        ctx.args = (static_kernel, dyadic_order, gram, nodes, _naive_solver, workspace_bytes)
        return _prefix_grid(_lib.get_backend(), static_kernel, X.detach(), Y.detach(), dyadic_order, _naive_solver, gram, workspace_bytes,
                            nodes)

    @staticmethod
    def backward(ctx, grad_output):
        X, Y, *params = ctx.saved_tensors
        static_kernel, d, gram, nodes, naive, workspace_bytes = ctx.args
        need_x, need_y = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        if X.shape[1] < 2 or Y.shape[1] < 2 or X.shape[0] == 0 or Y.shape[0] == 0:   # single points / empty batches: k = 1 whatever the paths
            gx, gy = (torch.zeros_like(X) if need_x else None), (torch.zeros_like(Y) if need_y else None)
            return (gx, gy, None, None, None, None, None, None) + _param_grads(params, None, ctx.needs_input_grad[8:])
        Xd, Yd = X.detach(), Y.detach()
        if nodes == "diagonal" and X.shape[1] != Y.shape[1]:
            T = min(X.shape[1], Y.shape[1])
            Xd, Yd = Xd[:, :T], Yd[:, :T]
        Mc, Nc = Xd.shape[1] - 1, Yd.shape[1] - 1
        go = grad_output.to(X.dtype)
        gx, gy, gp = _exact_gradient(_lib.get_backend(), static_kernel, Xd.contiguous(), Yd.contiguous(), None, d, naive, gram, workspace_bytes,
                                     need_x, need_y, sources=lambda a0, a1: _prefix_sources(go[a0:a1], nodes, Mc, Nc), params=params)
        if need_x and gx.shape != X.shape:
            gx = torch.cat((gx, torch.zeros_like(X[:, gx.shape[1]:])), dim=1)
        if need_y and gy.shape != Y.shape:
            gy = torch.cat((gy, torch.zeros_like(Y[:, gy.shape[1]:])), dim=1)
        return (gx, gy, None, None, None, None, None, None) + _param_grads(params, gp, ctx.needs_input_grad[8:])


def _repeat_last_point(P, lens):
    """P (batch, length, dim) with every point from lens[i] on overwritten by point lens[i] - 1 of its path (lens: int32 on P's device)"""
    idx = lens.long()
    last = P[torch.arange(P.shape[0], device=P.device), idx - 1]
    pad = torch.arange(P.shape[1], device=P.device)[None, :] >= idx[:, None]
    return torch.where(pad[:, :, None], last[:, None, :], P)


def k_kgrad(X, Y, gamma, dyadic_order, static_kernel, eps=1e-4, workspace_bytes=None):
    """Signature kernel and its first / second directional derivative along gamma -- the reference's ``k_kgrad``
    (sigkernel.py:504-593): X (A,M,D), Y (B,N,D), gamma (A,M,D) -> three (A,B) matrices
    k(x_a, y_b), d/ds k(x_a + s gamma_a, y_b)|_0, d2/ds2 k(x_a + s gamma_a, y_b)|_0.

    Like the reference, the derivatives of the static kernel are one-sided finite differences with step ``eps``
    (sigkernel.py:529-541; their truncation error is part of the reference's result, so it is reproduced, not
    "fixed"); the three increment arrays then drive ONE sweep of the coupled PDE stencil (cuda_backend.py:206-220)
    in sk_solve_deriv_*.  No autograd: the reference's outputs carry none either (solution buffers are fresh
    tensors, sigkernel.py:553-566).

    Function-valued paths (a static kernel with ``features``): the three node arrays are features(X), features(X + eps gamma) and
    features(X + 2 eps gamma) -- the perturbation is formed in input space, as the reference's Gram_matrix sees it (sigkernel.py:526-541)
    -- and the base kernel runs on them."""
    nodes = None
    if _functional(static_kernel):
        if gamma.shape != X.shape or gamma.dtype != X.dtype or gamma.device != X.device:
            raise ValueError("gamma must have X's shape, dtype and device")
        with torch.no_grad():
            phi = _FeatureMap(static_kernel)
            Xf, Yf = phi(X.detach()), phi(Y.detach())
            nodes = (phi(X.detach() + eps * gamma.detach()), phi(X.detach() + 2. * eps * gamma.detach()))
        X, Y, gamma, static_kernel = Xf, Yf, None, static_kernel.base_kernel
    _check_inputs(X, Y, paired=False)
    if gamma is not None and (gamma.shape != X.shape or gamma.dtype != X.dtype or gamma.device != X.device):
        raise ValueError("gamma must have X's shape, dtype and device")
    be = _lib.get_backend()
    A, B, M, N = X.shape[0], Y.shape[0], X.shape[1], Y.shape[1]
    out = torch.zeros(3, A, B, dtype=X.dtype, device=X.device)
    if M < 2 or N < 2:
        out[0] = 1.
        return out[0], out[1], out[2]
    # (contiguous once, here: X + eps gamma takes the strides of a strided view -- the staging of the HIP routes refuses that --, and a
    # static kernel evaluated by torch on a view may sum <x, y> in another order than on its contiguous copy)
    Xd, Yd, gd = X.detach().contiguous(), Y.detach().contiguous(), None if gamma is None else gamma.detach().contiguous()
    if nodes is not None:
        nodes = tuple(t.contiguous() for t in nodes)
    fused = _fused_static(static_kernel, True) if hasattr(be, "static_deriv_increments") else None
    # transient bytes per row of X: three increment arrays (+ three static Gram matrices on the generic route)
    per_row = (3 if fused is not None else 6) * B * M * N * X.element_size()
    for a0, a1 in _tiles(A, per_row, _budget(X.device, workspace_bytes)):
        Xt = Xd[a0:a1]
        if nodes is None:
            gt = gd[a0:a1]
            X1, X2 = Xt + eps * gt, Xt + 2. * eps * gt                               # sigkernel.py:530, :537
        else:
            X1, X2 = nodes[0][a0:a1], nodes[1][a0:a1]
        if fused is not None and hasattr(be, "solve_deriv_fused") and not routes.no_fused_deriv:
            # static kernel, finite differences, increments AND the three-state sweep in one kernel (sk_solve_deriv_static_f64)
            res = be.solve_deriv_fused(fused[0], fused[1], Xt.contiguous(), X1, X2, Yd.contiguous(), dyadic_order, eps)
            if res is not None:
                out[0, a0:a1], out[1, a0:a1], out[2, a0:a1] = res
                continue
        inc3 = None
        if fused is not None:    # static kernel + finite differences + increments in one pass (sk_static_deriv_increments_*)
            inc3 = be.static_deriv_increments(fused[0], fused[1], Xt.contiguous(), X1, X2, Yd.contiguous(), eps)
        if inc3 is None:
            G0 = static_kernel.Gram_matrix(Xt, Yd).contiguous()                      # :526
            G1 = static_kernel.Gram_matrix(X1, Yd).contiguous()                      # :530
            G2 = static_kernel.Gram_matrix(X2, Yd).contiguous()                      # :537
            inc3 = be.deriv_increments(G0, G1, G2, eps)                              # :527-541
            del G0, G1, G2
        k, kd, kdd = be.solve_deriv(inc3, dyadic_order)                              # :543-566 (tile() by index)
        out[0, a0:a1], out[1, a0:a1], out[2, a0:a1] = k, kd, kdd
    return out[0], out[1], out[2]


_SIDE_STREAMS = {}
_LOSS_WEIGHTS = {}


def _side_streams(device):
    """Two side streams per device, created once."""
    key = device.index if device.index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = (torch.cuda.Stream(device), torch.cuda.Stream(device))
    return _SIDE_STREAMS[key]


def routes_allow_streams():
    return not routes.no_mmd_streams


def _loss_weights(A, B, dtype, device, max_cached=16):
    """Constant weight matrices of the loss wrappers, built once per (A, B, dtype, device):
       wf (A, A+B)  value:    [ (1 - I) / (A (A-1)) | -2 / (A B) ]   -- K_XX_m - 2 mean(K_XY) = sum(K(X, [X; Y]) * wf)
       wb (A, A+B)  gradient: [ 2 (1 - I) / (A (A-1)) | -2 / (A B) ] -- d loss / dK with the reference's 2x rule on the K_XX part
                              (_SigKernelGram.backward doubles when both arguments require grad, sigkernel.py:410-412)
       wy (B, B)    value:    (1 - I) / (B (B-1))                     -- K_YY_m = sum(K_YY * wy); None for B < 2"""
    key = (A, B, dtype, device)
    capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
    ent = _LOSS_WEIGHTS.get(key)
    if ent is not None:
        # a captured hipGraph holds the cached tensors BY ADDRESS: an entry a capture has used is pinned for good (an eviction would
        # let the allocator hand its blocks out again under an already captured training step); everything else is least-recently-used
        _LOSS_WEIGHTS[key] = _LOSS_WEIGHTS.pop(key)[:3] + (ent[3] or capturing,)
        return ent[:3]
    # (built inside a hipGraph capture -- a capture without a warm-up call -- the fills are nodes of that graph and the memory
    # belongs to its pool: such weights serve the captured call only and are not cached)
    wf = torch.empty(A, A + B, dtype=dtype, device=device)
    wf[:, :A] = (1.0 - torch.eye(A, dtype=dtype, device=device)) / (A * (A - 1.0))
    wf[:, A:] = -2.0 / (A * float(B))
    wb = wf.clone()
    wb[:, :A] *= 2.0
    wy = (1.0 - torch.eye(B, dtype=dtype, device=device)) / (B * (B - 1.0)) if B > 1 else None
    w = (wf, wb, wy)
    if not capturing:
        if device.type == "cuda":
            torch.cuda.current_stream(device).synchronize()    # once per shape: later calls may read them from any stream
        _LOSS_WEIGHTS[key] = w + (False,)
        # bounded: workloads whose batch sizes vary would otherwise leak A (A + B) + B^2 elements per distinct shape; the oldest
        # UNPINNED entries go (dicts keep insertion order; a hit re-inserts its entry at the end)
        # (max_cached: weight sets kept besides those a graph capture has pinned)
        if len(_LOSS_WEIGHTS) > max_cached:
            for k in [k for k, e in _LOSS_WEIGHTS.items() if not e[3]][:len(_LOSS_WEIGHTS) - max_cached]:
                del _LOSS_WEIGHTS[k]
    return w


class _LossLaunch(NamedTuple):
    """What the one-launch loss forward (csrc/sk_loss.hip) leaves for its adjoint launch."""
    fused: tuple       # (kind, param) of the static kernel
    out: torch.Tensor       # the rectangle's values, then the triangle's
    edges: torch.Tensor
    staged: tuple      # (Zr, Zt, Zr_adj): [X; Y] as the kernels read it
    wb: torch.Tensor        # d value / dK of the rectangle's pairs
    A: int
    B: int
    M: int
    Yd: torch.Tensor


class _SigKernelLoss(torch.autograd.Function):
    """K_XX_m - 2 mean(K_XY) [+ K_YY_m] for TRAINING-SIZED batches: the value the reference's compute_mmd / compute_scoring_rule /
    compute_expected_scoring_rule (sigkernel.py:146-197) assemble from three (two) compute_Gram calls, from ONE Gram block
    K(X, Z), Z = [X; Y], and -- for the MMD -- the triangle of K(Y, Y).

    Why: a Gram matrix of a few thousand pairs is one wave's skew fill plus a pair or two per lane group, so the three forward and
    two adjoint launches of the reference's composition each leave most of the chip idle, and some sixty small launches (staging,
    reductions and their autograd) sit between them.  Here K_XX and K_XY are the column blocks of ONE forward launch (with the edges
    for backward) and their gradients ONE adjoint launch over the same pairs, weighted by the constant d loss / dK (_loss_weights;
    the reference's 2x rule for K_XX is in the weights); the reductions are two multiply-sums.  Same pairs, same kernels, same
    per-pair values; only the order in which the (A, A+B) values are summed differs from the reference's formula (last-bit).
    Without a gradient and with the K_YY term the whole triangle of K(Z, Z) is one launch."""

    @staticmethod
    def forward(ctx, X, Y, static_kernel, dyadic_order, _naive_solver, workspace_bytes, with_yy):
        be = _lib.get_backend()
        A, B = X.shape[0], Y.shape[0]
        Xd, Yd = X.detach().contiguous(), Y.detach().contiguous()
        ctx.static_kernel, ctx.dyadic_order, ctx._naive_solver, ctx.workspace_bytes = static_kernel, dyadic_order, _naive_solver, workspace_bytes
        ctx.kept = ctx.launch = None
        need = ctx.needs_input_grad[0]
        fast = _loss_launch_ok(be, static_kernel, Xd, Yd, dyadic_order, _naive_solver, need, with_yy, workspace_bytes)
        if fast is not None:
            # the one-launch glue (csrc/sk_loss.hip): staging of [X; Y] (no concatenated copy), K(X, [X; Y]) and the strict triangle of
            # K(Y, Y) in ONE forward launch, the scalar in one reduction -- three launches where the route below issues a dozen
            res = be.loss_forward(fast[0], fast[1], Xd, Yd, dyadic_order, _naive_solver, with_yy, keep_edges=need)
            if res is not None:
                val, out, edges, staged, wb = res
                if need:
                    ctx.save_for_backward(X)
                    ctx.launch = _LossLaunch(fast, out, edges, staged, wb, A, B, Xd.shape[1], Yd)
                return val
        Z = torch.cat((Xd, Yd))
        wf, wb, wy = _loss_weights(A, B, X.dtype, X.device)
        if not need and with_yy:
            K_ZZ = _gram_symmetric(be, static_kernel, Z, dyadic_order, _naive_solver, workspace_bytes)
            return (K_ZZ[:A] * wf).sum() + (K_ZZ[A:, A:] * wy).sum()
        # (K_YY on a side stream while a graph is captured -- compute_mmd's composition does that -- buys nothing here: replays of
        # 0.305 / 0.534 / 1.29 ms forked against 0.309 / 0.561 / 1.28 on one stream at 32 / 64 / 128 paths, tools/experiments/r04_merged_fork.py)
        K_YY = _gram_symmetric(be, static_kernel, Yd, dyadic_order, _naive_solver, workspace_bytes) if with_yy else None
        fused = _fused_static(static_kernel, True) is not None
        ctx.kept = _Kept() if need else None
        K_XZ = _gram_block(be, static_kernel, Xd, Z, dyadic_order, _naive_solver, workspace_bytes, (3 if fused else 8) if need else None,
                           ctx.kept)
        val = (K_XZ * wf).sum()
        if with_yy:
            val = val + (K_YY * wy).sum()
        if need:
            ctx.save_for_backward(X, Z)
            ctx.kept.K, ctx.wb = K_XZ, wb
        return val

    @staticmethod
    def backward(ctx, grad_output):
        be = _lib.get_backend()
        if ctx.launch is not None:
            # ONE fused adjoint over the rectangle's pairs, weighted by the constant d value / dK the forward's reduction left, from the
            # arrays the forward staged and the edges it kept; the upstream scalar stays on the device and multiplies the fold of the
            # partial sums into dL/dX (the adjoint is linear in it): screen + sweep + rescue + fold, four launches
            (X,) = ctx.saved_tensors
            L = ctx.launch      # (not taken off: the staged arrays serve every backward through a retained graph)
            (kind, param), (Zr, Zt, Zr_adj), wb, A, B = L.fused, L.staged, L.wb, L.A, L.B
            Xd = X.detach().contiguous()
            gs = grad_output.detach().to(torch.float64).contiguous()
            adj = be.linear_adjoint_fused if kind == 0 else be.rbf_adjoint_fused
            res = adj(Xd, None, param, ctx.dyadic_order, L.edges, wb, gram=True, kfinal=L.out[:A * (A + B)], naive=ctx._naive_solver,
                      staged=(Zr_adj, Zt, A + B, L.M), gscale=gs)
            if res is None:
                # sk_route_query named the one-band adjoint for this shape and its launcher declined all the same (a scope or workspace
                # check the query does not mirror): like every other gradient route, fall back -- the rows' gradient from the paths
                # (its own forward sweep; the kept edges are of no use to the streaming kernels) with the same weights
                go = (wb.view(A, A + B) * gs).contiguous()
                g = _rows_gradient(be, ctx.static_kernel, Xd, torch.cat((Xd, L.Yd)), go, ctx.dyadic_order, ctx._naive_solver, True, None,
                                   ctx.workspace_bytes)
                return g, None, None, None, None, None, None
            return res[0], None, None, None, None, None, None
        X, Z = ctx.saved_tensors
        go = (ctx.wb * grad_output.to(X.dtype)).contiguous()
        grad_X = _rows_gradient(be, ctx.static_kernel, X.detach().contiguous(), Z, go, ctx.dyadic_order, ctx._naive_solver, True, _take(ctx),
                                ctx.workspace_bytes)
        return grad_X, None, None, None, None, None, None


def _loss_launch_ok(be, static_kernel, Xd, Yd, dyadic, naive, need_grad, with_yy=True, workspace_bytes=None):
    """(kind, param) when a loss wrapper's call can take the one-launch glue of csrc/sk_loss.hip: exactly LinearKernel / RBFKernel,
    fp64 paths of one length, the ONE-BAND fused kernels for the forward and -- with a gradient pending -- for the adjoint too
    (sk_route_query on the rectangle's shape), pair counts inside the 32-bit / 15-bit fields of sk_solve_fwd_loss_f64 and
    sk_loss_value_f64 (checked HERE, before any launch), and -- with a gradient pending -- edges of the whole rectangle that fit the
    share of the transient budget a call may keep until backward (`keep_edges_fraction` of workspace_bytes, as _gram_block); None
    otherwise (the merged route's torch glue serves everything else: it tiles the rows and drops the edges where they do not fit)."""
    if routes.no_loss_launch or not hasattr(be, "loss_forward") or Xd.dtype != torch.float64 or Xd.shape[1:] != Yd.shape[1:]:
        return None
    fused = _fused_static(static_kernel, True)
    if fused is None:
        return None
    A, B, M = Xd.shape[0], Yd.shape[0], Xd.shape[1]
    tri_n = B if with_yy else 0
    p_rect, p_tri = A * (A + B), (tri_n * (tri_n - 1) // 2 if tri_n > 1 else 0)
    # sk_solve_fwd_loss_f64 packs A and tri_n into 15 bits each and indexes pairs with 31 bits; sk_loss_value_f64 indexes with 32
    if A > 0x7fff or tri_n > 0x7fff or p_rect >= 0x7ff00000 or p_rect + p_tri >= 0x7ff00000:
        return None
    if _route(be, OP_FORWARD, static_kernel, Xd, Yd, dyadic, naive, True) != FUSED:
        return None
    if need_grad and _route(be, OP_ADJOINT, static_kernel, Xd, Yd, dyadic, naive, True) != FUSED:
        return None
    # what the call allocates in one piece and (the edges, the weights, the staged paths) holds until backward: 8 (MM + NN + 32)
    # bytes of edges per rectangle pair, values + weights + pair table 8 bytes per pair each
    held = 8.0 * p_rect * ((2 * ((M - 1) << int(dyadic)) + 32) if need_grad else 0) + 8.0 * (3 * p_rect + 2 * p_tri)
    if (workspace_bytes is not None or held > _cost("loss_launch_free_bytes")) and \
            held > _cost("keep_edges_fraction") * _budget(Xd.device, workspace_bytes):
        return None
    return fused


_LOSS_LAUNCH_FREE_BYTES = None    # "loss_launch_free_bytes": below this the one-launch loss route does not ask the device for its free memory


def _prefix_nodes(grid, nodes):
    """the slice `nodes` of prefix grids (..., M, N): their diagonal (..., min(M, N)), last row (..., N) or last column (..., M)"""
    if nodes == "diagonal":
        return torch.diagonal(grid, dim1=-2, dim2=-1)
    return grid[..., -1, :] if nodes == "last_row" else grid[..., :, -1]


def _prefix_grid(be, static_kernel, Xd, Yd, dyadic, naive, gram, workspace_bytes, nodes="all"):
    """out[..., m, n] = k_sig(x[:m+1], y[:n+1]) for every pair: (A, B, M, N) for gram, (A, M, N) paired.  The fused prefix kernel where the
    library says so (sk_route_query(SK_OP_PREFIX): no transient memory), else the existing pieces -- increments, the streaming
    solver's full grid, its coarse nodes -- over row tiles that keep increments + fine grid within the budget.
    nodes = "diagonal" / "last_row" / "last_col": only that slice of every grid, (..., min(M, N)) / (..., N) / (..., M) -- stored alone by
    the fused kernel, taken from each row tile's grid elsewhere: nothing of size pairs x M x N is allocated beyond a tile."""
    A, M, N = Xd.shape[0], Xd.shape[1], Yd.shape[1]
    B = Yd.shape[0] if gram else 1
    tail = (M, N) if nodes == "all" else (_lib.prefix_nodes_len(nodes, M, N),)
    shape = ((A, Yd.shape[0]) if gram else (A,)) + tail
    if M < 2 or N < 2 or A == 0 or B == 0:      # one-point paths: every prefix kernel is 1; empty batches: empty results
        return torch.ones(shape, dtype=Xd.dtype, device=Xd.device)
    fused = _fused_static(static_kernel, gram)
    if fused is not None and hasattr(be, "solve_prefix_fused") and not routes.no_fused_prefix and \
            not (fused[0] == 1 and routes.no_fused_rbf):
        # (the back-end asks sk_route_query(SK_OP_PREFIX) and returns None where the library names the streamed route)
        more = {} if nodes == "all" else {"nodes": nodes}
        out = be.solve_prefix_fused(fused[0], fused[1], Xd.contiguous(), Yd.contiguous(), dyadic, naive, gram, **more)
        if out is not None:
            return out
    out = torch.empty(shape, dtype=Xd.dtype, device=Xd.device)
    r = 1 << dyadic
    # per row of the tile: the increments (padded rows) and the fine grid the streaming solver writes
    per_row = B * ((M - 1) * (N + 16) + (((M - 1) << dyadic) + 1) * (((N - 1) << dyadic) + 1)) * Xd.element_size()
    for a0, a1 in _tiles(A, per_row, _budget(Xd.device, workspace_bytes)):
        inc = _increments(be, static_kernel, Xd[a0:a1], Yd if gram else Yd[a0:a1], gram=gram)
        _, grid, _ = be.solve_fwd(inc, dyadic, naive, want_grid=True)
        out[a0:a1] = grid[..., ::r, ::r] if nodes == "all" else _prefix_nodes(grid[..., ::r, ::r], nodes)
        del inc, grid
    return out


def _prefix_at(be, static_kernel, Xd, Yd, lx, ly, dyadic, naive, gram, workspace_bytes):
    """out[a, b] = k_sig(x_a[:lx[a]], y_b[:ly[b]]) -- (A, B) for gram, (A,) paired -- for paths padded at their ends to common lengths;
    lx / ly: validated int32 lengths on the paths' device.  The fused prefix kernel storing ONE node per pair where the library says so
    (sk_route_query(SK_OP_PREFIX); the same `routes` switches as _prefix_grid): nothing of size pairs x M x N exists.  Else, over row
    tiles within the budget: increments, the table {lx - 1, ly - 1} of the tile's pairs, and be.solve_fwd_at -- one node per pair again,
    no fine grid; by default every pair's own sub-grid on the anti-diagonal kernel (bit for bit the node of the stored grid), with
    `routes.ragged_stream` the streaming kernel where it serves the shape.  A back-end without solve_fwd_at, or
    `routes.no_ragged_nodes`: the pieces of _prefix_grid's fallback -- increments, the solver's full fine grid, its coarse nodes --
    with the node of every pair gathered from a tile's grid before the tile is dropped."""
    A, M, N = Xd.shape[0], Xd.shape[1], Yd.shape[1]
    B = Yd.shape[0] if gram else 1
    shape = (A, Yd.shape[0]) if gram else (A,)
    if M < 2 or N < 2 or A == 0 or B == 0:      # one-point paths: every kernel is 1; empty batches: empty results
        return torch.ones(shape, dtype=Xd.dtype, device=Xd.device)
    fused = _fused_static(static_kernel, gram)
    if fused is not None and hasattr(be, "solve_prefix_at") and not routes.no_fused_prefix and \
            not (fused[0] == 1 and routes.no_fused_rbf):
        # (the back-end asks sk_route_query(SK_OP_PREFIX) and returns None where the library names the streamed route)
        out = be.solve_prefix_at(fused[0], fused[1], Xd.contiguous(), Yd.contiguous(), lx, ly, dyadic, naive, gram)
        if out is not None:
            return out
    out = torch.empty(shape, dtype=Xd.dtype, device=Xd.device)
    if hasattr(be, "solve_fwd_at") and not routes.no_ragged_nodes:
        # one node per pair and no fine grid: per row of the tile the increments (padded rows) and the table {mc, nc} alone.  By default
        # the anti-diagonal kernel over every pair's own sub-grid (the bits of the stored grid's node, at the cost of the true lengths);
        # routes.ragged_stream: the streaming kernel where it serves the shape (dyadic orders above 3 stay on the anti-diagonal kernel)
        flags = 0 if routes.ragged_stream else _lib.FLAG_SIMPLE
        cx, cy = lx.to(torch.int32) - 1, ly.to(torch.int32) - 1
        per_row = B * ((M - 1) * (N + 16) * Xd.element_size() + 8)
        for a0, a1 in _tiles(A, per_row, _budget(Xd.device, workspace_bytes)):
            inc = _increments(be, static_kernel, Xd[a0:a1], Yd if gram else Yd[a0:a1], gram=gram)
            if gram:
                cells = torch.stack((cx[a0:a1, None].expand(a1 - a0, B), cy[None, :].expand(a1 - a0, B)), dim=-1)
            else:
                cells = torch.stack((cx[a0:a1], cy[a0:a1]), dim=-1)
            out[a0:a1] = be.solve_fwd_at(inc, cells, dyadic, naive, flags)
            del inc, cells
        return out
    r = 1 << dyadic
    ix, iy = lx.long() - 1, ly.long() - 1
    per_row = B * ((M - 1) * (N + 16) + (((M - 1) << dyadic) + 1) * (((N - 1) << dyadic) + 1)) * Xd.element_size()
    for a0, a1 in _tiles(A, per_row, _budget(Xd.device, workspace_bytes)):
        inc = _increments(be, static_kernel, Xd[a0:a1], Yd if gram else Yd[a0:a1], gram=gram)
        _, grid, _ = be.solve_fwd(inc, dyadic, naive, want_grid=True)
        coarse = grid[..., ::r, ::r]
        rows = torch.arange(a1 - a0, device=Xd.device)
        if gram:
            out[a0:a1] = coarse[rows[:, None], torch.arange(B, device=Xd.device)[None, :], ix[a0:a1, None], iy[None, :]]
        else:
            out[a0:a1] = coarse[rows, ix[a0:a1], iy[a0:a1]]
        del inc, grid, coarse
    return out


class _Lengths:
    """Lengths that _lengths has checked: the int32 tensor on the paths' device and the host copy (one transfer, one check per call of a
    public method, however many Gram matrices it takes)."""
    __slots__ = ("dev", "host", "count", "padded")

    def __init__(self, name, lens, count, padded, device):
        self.count, self.padded = count, padded
        self.dev, self.host = _lengths(name, lens, count, padded, device, True)


def _lengths(name, lens, count, padded, device, with_host=False):
    """The point counts of a ragged batch, checked ONCE on the host -- `count` integers in [1, padded] -- and returned as a contiguous
    int32 tensor on `device`.  ValueError naming the argument otherwise.  A _Lengths (already checked) passes through."""
    if isinstance(lens, _Lengths):
        if lens.count != count or lens.padded != padded:
            raise ValueError("%s: %d lengths checked against a padded length of %d do not fit %d paths of %d points"
                             % (name, lens.count, lens.padded, count, padded))
        return lens.dev
    t = lens if torch.is_tensor(lens) else torch.as_tensor(list(lens))
    if t.numel() == 0 and not torch.is_tensor(lens):
        t = t.to(torch.int64)
    if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError("%s must hold integers (an integer tensor or a sequence of ints), not %s" % (name, t.dtype))
    if t.dim() != 1 or t.shape[0] != count:
        raise ValueError("%s must hold one length per path: expected shape (%d,), got %s" % (name, count, tuple(t.shape)))
    host = t.detach().to("cpu", torch.int64)
    if count and (int(host.min()) < 1 or int(host.max()) > padded):
        raise ValueError("%s must lie in [1, %d] (the padded length), got values from %d to %d" % (name, padded, int(host.min()), int(host.max())))
    dev = host.to(torch.int32).to(device).contiguous()
    return (dev, host) if with_host else dev


def pad_paths(paths):
    """A list of (len_i, dim) tensors -> (X (batch, max len, dim), lens (batch,) int64): every path padded at its END by repeating its
    last point, for ``SigKernel.compute_Gram_ragged`` / ``compute_kernel_ragged`` / ``compute_mmd_ragged`` (whose values never depend
    on the padding, and whose gradients under ``exact_gradient=True`` are exactly zero on it: any values would do, NaN and inf included).  ``X[i, :lens[i]]`` is path i again."""
    paths = list(paths)
    if not paths:
        raise ValueError("pad_paths needs at least one path")
    for p in paths:
        if not torch.is_tensor(p) or p.dim() != 2 or p.shape[0] < 1:
            raise ValueError("every path must be a tensor of shape (length >= 1, dim)")
        if p.shape[1] != paths[0].shape[1] or p.dtype != paths[0].dtype or p.device != paths[0].device:
            raise ValueError("all paths must share dim, dtype and device")
    lens = torch.tensor([p.shape[0] for p in paths], dtype=torch.int64)
    L = int(lens.max())
    X = torch.stack([torch.cat((p, p[-1:].expand(L - p.shape[0], -1))) for p in paths])
    return X, lens


class _NoGradCtx:
    """What the autograd Functions' forward needs of a context when no gradient can be asked for: the call skips
    torch.autograd.Function.apply (a quarter of the host time of a C1-sized call) and returns the same values."""
    needs_input_grad = (False,) * 8

    def save_for_backward(self, *tensors):
        pass


def _wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class SigKernelStream:
    """Complete paths X scored against streams that GROW: ``SigKernel.open_stream(X, Y0)`` -> this, ``append(Ynew)`` -> the kernels
    of X against every new prefix, in time linear in the stream.

    X (A, M, D): the bank of complete paths.  Y0 (B, n0 >= 1, D): what the B streams hold so far.  ``paired=True``: stream a runs
    against bank path a (B == A) and the pair axis below is one axis (A,) instead of (A, B).

      ``append(Ynew)``   Ynew (B, c, D), the next c points of every stream -> (A, B, c): k(x_a, y_b[:n + 1]) for each NEW point n, in
                         order -- bit for bit ``compute_Gram_prefixes(X, all of y, nodes="last_row")[..., -c:]``.  c == 0: an empty
                         (A, B, 0) tensor.  Values in the dtype of the paths, no ``grad_fn``.
      ``kernel``         (A, B): k(x_a, y_b) as the streams stand, ``compute_Gram(X, all of y)`` bit for bit
      ``length``         points seen per stream
      ``resumes``        True: every append sweeps only its new points (below); False: every append sweeps the whole history
      ``state_bytes``    bytes the stream holds between appends (below)
      ``route``          "fused", "column" or "history": what an append runs (below; read-only)

    ``resumes``: inside the fused prefix kernel's scope (exactly LinearKernel / RBFKernel, dim <= 8, dyadic_order <= 2, bank paths of one
    band, the library back-end) all that crosses a column of a pair's PDE grid is that column, so the stream keeps one fine column per
    pair -- fp64 whatever the paths' dtype -- and an append launches ONE sweep of the prefix kernel over the new points that starts
    from it (csrc/sk_wave_prefix.hip, RESUME).  The kept column sits at an even point of the stream; the one or two points behind it
    are kept too and swept again with the next chunk (at most one column more per append).  The bank is staged once, when the
    stream is opened.  ``state_bytes`` = the two column arrays the sweeps alternate between (2 x pairs x pitch x 8 bytes, pitch = the bank
    paths' fine rows rounded up to whole lanes) + the staged bank + the kept points: constant in the stream's length.  A launch has
    a fixed cost of about as many macro-steps as a bank path has lanes, so appending point by point is far from free: see README.md
    for the chunk size from which an append beats sweeping the history again.

    Outside that scope (dim > 8, bank paths of more than one band, dyadic_order > 2, duck-typed or function-valued static kernels,
    ``routes.no_fused_prefix``, a back-end without ``solve_prefix_resume``) the stream keeps its HISTORY and every append is
    ``compute_Gram_prefixes(X, history, nodes="last_row")`` over all of it: the same values, time quadratic in the stream;
    ``state_bytes`` = the history's bytes and grows with it.

    ``resume="always"`` (``open_stream(X, Y0, resume="always")``; the default is ``"fused"``, the behaviour above) resumes outside that
    scope as well -- the column route, ``route == "column"``, ``resumes`` True.  Off the fused scope the values come from the
    anti-diagonal solver (csrc/sk_simple.hip), which sweeps in fp64 and evaluates every cell from the same operands in the same order
    whatever the grid's extent: a sweep over a piece of y that takes its left boundary from the kept fine column instead of the
    constant 1 reproduces the one-shot sweep's cells bit for bit (``sk_solve_fwd_resume_*``, a launch-time mode of the same kernel).
    A kernel of function-valued paths is its ``base_kernel`` on the features (as in every other method): under "always" its stream is
    the stream of the features -- the bank mapped once at open, every piece as it arrives -- and so takes the fused resume where the
    FEATURES lie in the fused scope (RBF_ID_Kernel on (4, 2)-valued points: dim 8, ``route == "fused"``, the route whose bits the one-shot
    call on such paths has) and the column route elsewhere.
    The stream keeps the bank (function-valued kernels: its features), two fp64 column arrays
    (pairs, ((M - 1) << dyadic_order) + 1) that the sweeps alternate between, and the streams' last point: ``state_bytes`` is their sum,
    constant in the stream's length.  An append forms the increments of the piece [last point] + Ynew alone (row-tiled under
    ``workspace_bytes``), one launch per tile, and returns the coarse nodes of the terminal row.  Any path dim, dyadic order and static
    kernel; the bank's fine rows must fit the solver's LDS limit (3 x 8 x (((M - 1) << dyadic_order) + 1) bytes within 160 KiB), and the
    back-end must have ``solve_fwd_resume`` -- else the stream keeps its history as under "fused" (``route == "history"``).  Inside
    the fused scope "always" is the fused resume (``route == "fused"``).  Bits: exactly LinearKernel / RBFKernel, and Linear_ID_Kernel /
    RBF_ID_Kernel / RBF_SQR_Kernel over them, give ``compute_Gram_prefixes(X, y, nodes="last_row")`` bit for bit -- an increment of a
    piece is computed from its own two points of y alone, and these feature maps act on each time point alone, element by element.
    RBF_CEXP_Kernel's ``features`` is a matmul along the space axis: also each time point alone, so it takes the column route, but the
    matmul's rounding may depend on how many points it maps at once; a duck-typed kernel's ``Gram_matrix`` likewise.  Those agree with
    the one-shot call to rounding (1e-12 relative in fp64), not to the bit.  No feature map of static_kernels.py mixes time points;
    a user-defined one that does must not be streamed with "always".  Thin chunks fill few of the solver's 64 lanes (an
    anti-diagonal of a piece of c points has at most c << dyadic_order cells): see README.md for the measured chunk sizes.

    Forward only: an input that requires grad raises ``NotImplementedError`` (outside ``torch.no_grad()``), on ``exact_gradient=True``
    objects too, whose forward values are the same.  Not sharded (``process_group`` raises).  Only the streams grow: a bank whose
    paths grow as well would need the kept last ROW too."""

    def __init__(self, sk, X, Y0, paired=False, resume="fused"):
        if resume not in ("fused", "always"):
            raise ValueError("resume must be 'fused' or 'always', not %r" % (resume,))
        if sk.process_group is not None:
            raise NotImplementedError("streams are not sharded over a process group; open the stream on a SigKernel without process_group")
        self._sk, self._gram = sk, not paired
        raw = _functional(sk.static_kernel)      # (function-valued paths: (batch, length, Lx, d); the feature map checks them)
        if not raw:
            _check_inputs(X, Y0, paired=paired)
        if Y0.shape[1] < 1:
            raise ValueError("Y0 must hold at least one point per stream")
        if _wants_grad(X, Y0, *_static_params(sk.static_kernel)):
            raise NotImplementedError("streams are forward only: open them under torch.no_grad() or on detached paths")
        self._X = X.detach()
        self._tail_shape = tuple(Y0.shape[2:])
        self._B, self.length = Y0.shape[0], 0
        self._pairs_shape = (X.shape[0], Y0.shape[0]) if self._gram else (X.shape[0],)
        self._col, self._cur, self._bank, self._tail, self._hist, self._kernel = None, None, None, None, None, None
        self._column, self._on = False, None
        if raw and resume == "always":
            # a kernel of function-valued paths IS its base kernel on the features (SigKernel._on_features): the stream of the features,
            # bank mapped once here, every piece as it arrives -- the fused resume where the features lie in its scope, else the column
            inner = SigKernel(sk.static_kernel.base_kernel, sk.dyadic_order, sk._naive_solver, sk.workspace_bytes, None, sk.exact_gradient)
            with torch.no_grad():
                self._on = SigKernelStream(inner, sk.static_kernel.features(self._X), sk.static_kernel.features(Y0.detach()), paired, resume)
            self.resumes, self.length = self._on.resumes, self._on.length
            return
        be = _lib.get_backend()
        fused = None if raw else _fused_static(sk.static_kernel, self._gram)
        self.resumes = bool(
            fused is not None and hasattr(be, "solve_prefix_resume") and hasattr(be, "route") and not routes.no_fused_prefix
            and not (fused[0] == 1 and routes.no_fused_rbf) and X.shape[0] > 0 and Y0.shape[0] > 0 and X.shape[1] >= 2
            and _route_query(be.route, _lib.OP_PREFIX, fused[0], X.shape[2], X.shape[1], 2, sk.dyadic_order, bool(sk._naive_solver),
                             X.element_size()) == FUSED)
        if self.resumes:
            self._fused = fused
            self._X = self._X.contiguous()
            self._bank = be.stage_prefix_bank(fused[0], fused[1], self._X, sk.dyadic_order, self._gram)
            pairs = X.shape[0] * (Y0.shape[0] if self._gram else 1)
            pitch = be.state_pitch(fused[0], X.shape[1], sk.dyadic_order)
            self._col = [torch.empty((pairs, pitch), dtype=torch.float64, device=X.device) for _ in range(2)]
            self._kernel = torch.ones(self._pairs_shape, dtype=X.dtype, device=X.device)
        self._column = bool(
            resume == "always" and not self.resumes and hasattr(be, "solve_fwd_resume") and X.shape[0] > 0 and Y0.shape[0] > 0
            and X.shape[1] >= 2 and (not hasattr(be, "resume_fits") or be.resume_fits(X.shape[1], sk.dyadic_order)))
        if self._column:
            # the column route: the anti-diagonal solver resumed from a kept fine column, behind any static kernel
            self.resumes = True
            self._bank = self._X.contiguous()
            pairs = X.shape[0] * (Y0.shape[0] if self._gram else 1)
            fine = ((X.shape[1] - 1) << sk.dyadic_order) + 1
            self._col = [torch.ones((pairs, fine), dtype=torch.float64, device=X.device),
                         torch.empty((pairs, fine), dtype=torch.float64, device=X.device)]
            self._cur = 0
            self._kernel = torch.ones(self._pairs_shape, dtype=X.dtype, device=X.device)
        self._push(Y0.detach(), first=True)

    def _check(self, Ynew):
        X = self._X
        if not torch.is_tensor(Ynew) or Ynew.dim() != X.dim() or tuple(Ynew.shape[2:]) != self._tail_shape:
            raise ValueError("Ynew must have shape (%d, c, %s): the streams' next c points" % (self._B, ", ".join(str(d) for d in self._tail_shape)))
        if Ynew.shape[0] != self._B:
            raise ValueError("Ynew must hold the next points of all %d streams, got a batch of %d" % (self._B, Ynew.shape[0]))
        if Ynew.dtype != X.dtype or Ynew.device != X.device:
            raise ValueError("Ynew must share dtype and device with the paths the stream was opened on (%s on %s)" % (X.dtype, X.device))
        if _wants_grad(Ynew):
            raise NotImplementedError("streams are forward only: append under torch.no_grad() or detached points")

    def _push(self, Ynew, first=False):
        """the kernels of the c new points, (pairs..., c); first: Ynew opens the streams (its first point has the kernel 1)"""
        c = Ynew.shape[1]
        self.length += c
        if not self.resumes:
            self._hist = Ynew.contiguous() if first else torch.cat((self._hist, Ynew), dim=1)
            call = self._sk.compute_Gram_prefixes if self._gram else self._sk.compute_kernel_prefixes
            with torch.no_grad():
                row = call(self._X, self._hist, nodes="last_row")
            self._kernel = row[..., -1]
            return row[..., row.shape[-1] - c:]
        if self._column:
            return self._push_column(Ynew, first)
        # the one or two points behind the kept column, then the new ones: the piece the sweep resumes over
        piece = Ynew.contiguous() if first else torch.cat((self._tail, Ynew), dim=1)
        kept = 0 if first else self._tail.shape[1]
        if piece.shape[1] < 2:      # one point in all: nothing to sweep yet
            self._tail = piece
            return self._kernel[..., None].clone()
        be, sk = _lib.get_backend(), self._sk
        col_in = None if self._cur is None else self._col[self._cur]
        nxt = 0 if self._cur is None else 1 - self._cur
        res = be.solve_prefix_resume(self._fused[0], self._fused[1], self._X, piece, sk.dyadic_order, sk._naive_solver, self._gram,
                                     col_in, self._col[nxt], bank=self._bank)
        if res is None:
            raise RuntimeError("the prefix kernel refused a resumed launch inside its own scope (sk_solve_prefix_resume_*)")
        row, advanced = res
        if advanced:
            self._cur = nxt
        self._tail = piece[:, advanced:].contiguous()
        self._kernel = row[..., -1].clone()
        if first:
            row[..., 0] = 1       # k against a one-point prefix
            return row
        return row[..., kept:]

    def _push_column(self, Ynew, first):
        """the column route's append: the increments of the piece [last point] + Ynew alone -- c coarse columns --, one
        solve_fwd_resume launch per row tile from the kept fine column, the coarse nodes of the terminal row"""
        be, sk = _lib.get_backend(), self._sk
        X, d = self._bank, sk.dyadic_order
        piece = Ynew.contiguous() if first else torch.cat((self._tail, Ynew), dim=1)
        self._tail = piece[:, -1:].clone()      # the streams' last point
        c = piece.shape[1] - 1
        if c == 0:      # a first chunk of one point: nothing to sweep, the column of ones stands
            return self._kernel[..., None].clone()
        A, M, B, r = X.shape[0], X.shape[1], (self._B if self._gram else 1), 1 << d
        col_in, col_out = self._col[self._cur], self._col[1 - self._cur]
        out = torch.empty(self._pairs_shape + (c,), dtype=X.dtype, device=X.device)
        # per row of the tile: the increments of the piece (padded rows) and the fp64 terminal row; the columns are pair-major, so a
        # row tile is a contiguous slice of them
        per_row = B * ((M - 1) * (c + 16) * X.element_size() + 8 * ((c << d) + 1))
        for a0, a1 in _tiles(A, per_row, _budget(X.device, sk.workspace_bytes)):
            inc = _increments(be, sk.static_kernel, X[a0:a1], piece if self._gram else piece[a0:a1], gram=self._gram)
            row = be.solve_fwd_resume(inc, d, sk._naive_solver, col_in[a0 * B:a1 * B], col_out[a0 * B:a1 * B])
            out[a0:a1] = row[..., r::r]      # nodes (1..c) << d, rounded to the paths' dtype as a stored grid's are
            del inc, row
        self._cur = 1 - self._cur
        self._kernel = out[..., -1].clone()
        if first:      # k against a one-point prefix, then the swept nodes
            return torch.cat((torch.ones_like(out[..., :1]), out), dim=-1)
        return out

    def append(self, Ynew):
        """Ynew (B, c, D): the streams' next c points -> (A, B, c) ((A, c) paired): k(x_a, y_b[:n + 1]) for every new point, in order."""
        self._check(Ynew)
        if Ynew.shape[1] == 0:
            return torch.empty(self._pairs_shape + (0,), dtype=self._X.dtype, device=self._X.device)
        if self._on is not None:      # function-valued paths under resume="always": the piece's features, as they arrive
            with torch.no_grad():
                new = self._on.append(self._sk.static_kernel.features(Ynew.detach()))
            self.length = self._on.length
            return new
        return self._push(Ynew.detach())

    @property
    def kernel(self):
        """(A, B) ((A,) paired): k(x_a, y_b) as the streams stand -- ``compute_Gram(X, all of y)`` bit for bit"""
        return self._kernel if self._on is None else self._on.kernel

    @property
    def route(self):
        """"fused": the prefix kernel resumed from its kept column; "column": the anti-diagonal solver resumed from a kept fine column
        (``resume="always"`` off the fused scope); "history": every append sweeps the kept history again"""
        if self._on is not None:
            return self._on.route
        return "column" if self._column else "fused" if self.resumes else "history"

    @property
    def state_bytes(self):
        if self._on is not None:
            return self._on.state_bytes
        held = [self._hist] if not self.resumes else list(self._col) + [self._bank, self._tail]
        return sum(t.numel() * t.element_size() for t in held if t is not None)


class SigKernel:
    """Signature kernel k_sig(x, y) = <S(f(x)), S(f(y))> for a static kernel k(x, y) = <f(x), f(y)>.

    Drop-in for the reference's ``SigKernel`` (sigkernel.py:15-197): same constructor, same methods,
    same shapes / dtypes / devices.  Tensors must live on a HIP device (``'cuda'`` in PyTorch-ROCm).

    Extra, optional: ``workspace_bytes`` bounds the transient HBM a call may use (default: half of
    the free memory, at most 48 GiB); ``process_group`` shards ``compute_Gram`` rows over the ranks
    of a ``torch.distributed`` group (see :mod:`sigkernel_amd.distributed`).

    ``exact_gradient`` (default False): which gradient ``backward`` returns.  False: the reference's adjoint formula
    ``sum K[i][j] K~[i+1][j+1] d inc[i][j]`` -- the continuous PDE's, the parity contract; it is NOT the derivative of the number the
    forward pass computes (tens of per cent away at dyadic orders 0..2, so ``torch.autograd.gradcheck`` fails), only X receives it, and
    ``compute_Gram(X, X)`` relies on the reference's 2x rule.  True: the exact adjoint of the discrete solver ("Exact
    gradient"): forward values as ever, on whatever route they take; X AND Y receive the true gradient of those values (no 2x rule:
    where X is Y autograd adds the two), ``compute_mmd`` / ``compute_distance`` / the scoring rules become compositions of
    ``compute_Gram`` / ``compute_kernel`` and accept a Y that requires grad.  The backward solves every pair with the stored-grid
    kernel (a few times the cost of the default's fused adjoints) and runs in fp64: fp32 paths are up-cast for it and their gradients
    rounded to fp32 at the end.  Ragged batches (``compute_Gram_ragged`` / ``compute_kernel_ragged`` / ``compute_mmd_ragged``) get
    their gradients in this mode and in this mode only: every pair's backward sweeps its own sub-grid, and the padding -- any
    values, NaN and inf included -- receives exactly zero.  The prefix methods (``compute_Gram_prefixes`` /
    ``compute_kernel_prefixes`` in every ``nodes`` mode, ``compute_mmd_prefixes``) likewise: one reverse sweep per pair differentiates any
    weighting of a pair's prefix kernels -- a loss over time costs one backward, not one per time.  Not sharded (``process_group`` raises
    ``NotImplementedError``).  The static kernel's own parameters are differentiated too: ``RBFKernel(sigma)`` with ``sigma`` a one-element
    tensor that requires grad gets ``sigma.grad`` (up to 32 dims from the same HIP launch that gives X its gradient), a static kernel
    that is a ``torch.nn.Module`` gets its parameters' gradients through one vector-Jacobian product; a call where only such a
    parameter requires grad is differentiated like any other.  A default object reads a tensor ``sigma`` as its value.
    """

    def __init__(self, static_kernel, dyadic_order, _naive_solver=False, workspace_bytes=None, process_group=None, exact_gradient=False):
        if exact_gradient and process_group is not None:
            raise NotImplementedError("exact_gradient=True is not sharded over a process group; use a SigKernel without process_group")
        self.static_kernel = static_kernel
        self.dyadic_order = dyadic_order
        self._naive_solver = _naive_solver
        self.workspace_bytes = workspace_bytes
        self.process_group = process_group
        self.exact_gradient = bool(exact_gradient)

    def _params(self):
        """The static kernel's tensors this object differentiates (_static_params) -- under exact_gradient=True; a default object
        reads a tensor sigma as its value."""
        return _static_params(self.static_kernel) if self.exact_gradient else ()

    def _on_features(self):
        """(SigKernel of the base kernel, feature map) when the static kernel is one of function-valued paths, else None: the one
        dispatch point of the methods below.  Inputs are mapped once each and the method runs on the features; gradients reach the
        paths through torch autograd of the feature map."""
        if not _functional(self.static_kernel):
            return None
        inner = SigKernel(self.static_kernel.base_kernel, self.dyadic_order, self._naive_solver, self.workspace_bytes, self.process_group,
                          self.exact_gradient)
        return inner, _FeatureMap(self.static_kernel)

    def open_stream(self, X, Y0, paired=False, resume="fused"):
        """X (A, M, D) complete paths, Y0 (B, n0 >= 1, D) what B streams hold so far -> a :class:`SigKernelStream`: ``append(Ynew)``
        returns k(x_a, y_b[:n + 1]) for every new point of the streams -- ``compute_Gram_prefixes(X, y, nodes="last_row")`` as y
        arrives, bit for bit, without sweeping the history again.  ``paired=True``: stream a against bank path a.
        ``resume``: "fused" (default) resumes inside the fused prefix kernel's scope only and keeps the history elsewhere; "always"
        resumes outside that scope too, from a kept fine column of the anti-diagonal solver (``route == "column"``: any path dim, bank
        length within the solver's LDS limit, dyadic order and static kernel; see :class:`SigKernelStream`).  Any other string raises
        ``ValueError``."""
        return SigKernelStream(self, X, Y0, paired, resume)

    def compute_kernel(self, X, Y, max_batch=100):
        """X (batch, len_x, dim), Y (batch, len_y, dim) -> (batch,) vector k(X^i_T, Y^i_T).

        ``max_batch`` is kept for signature compatibility (sigkernel.py:23); tiling is by HBM budget.  Under a process group the
        pairs are sharded over the ranks like Gram rows (sigkernel_amd.distributed.ShardedPaired)."""
        f = self._on_features()
        if f is not None:
            return f[0].compute_kernel(f[1](X), f[1](Y), max_batch)
        if self.process_group is not None:
            from .distributed import sharded_kernel
            return sharded_kernel(self, X, Y, self.process_group)
        params = self._params()
        if not _wants_grad(X, Y, *params):
            return _SigKernel.forward(_NoGradCtx(), X, Y, self.static_kernel, self.dyadic_order, self._naive_solver, self.workspace_bytes)
        if self.exact_gradient:
            return _SigKernelExact.apply(X, Y, self.static_kernel, self.dyadic_order, False, False, self._naive_solver, self.workspace_bytes,
                                         *params)
        return _SigKernel.apply(X, Y, self.static_kernel, self.dyadic_order, self._naive_solver, self.workspace_bytes)

    def _prefixes(self, X, Y, gram, max_batch, nodes="all"):
        if nodes not in _lib.PREFIX_NODES:
            raise ValueError("nodes must be one of %s, not %r" % (", ".join(repr(n) for n in _lib.PREFIX_NODES), nodes))
        f = self._on_features()
        if f is not None:
            return f[0]._prefixes(f[1](X), f[1](Y), gram, max_batch, nodes)
        _check_inputs(X, Y, paired=not gram)
        if self.process_group is not None:
            raise NotImplementedError("prefix grids are not sharded over a process group: every rank would have to gather an "
                                      "(A, B, M, N) tensor; call it on a SigKernel without process_group")
        params = self._params()
        if _wants_grad(X, Y, *params):
            if not self.exact_gradient:
                raise NotImplementedError("compute_Gram_prefixes / compute_kernel_prefixes are forward only on this object: the "
                                          "reference's adjoint formula has no prefix form.  Construct the SigKernel with "
                                          "exact_gradient=True for their true gradient, or call them under torch.no_grad() or on "
                                          "detached paths")
            return _SigKernelPrefixExact.apply(X, Y, self.static_kernel, self.dyadic_order, gram, nodes, self._naive_solver,
                                               self.workspace_bytes, *params)
        return _prefix_grid(_lib.get_backend(), self.static_kernel, X.detach(), Y.detach(), self.dyadic_order, self._naive_solver, gram,
                            self.workspace_bytes, nodes)

    def compute_Gram_prefixes(self, X, Y, max_batch=100, nodes="all"):
        """X (batch_X, len_x, dim), Y (batch_Y, len_y, dim) -> (batch_X, batch_Y, len_x, len_y): out[a, b, m, n] =
        k(X^a restricted to its first m + 1 points, Y^b restricted to its first n + 1 points) -- the coarse nodes of the PDE grid the
        solver sweeps anyway (node (m << dyadic_order, n << dyadic_order) of the reference's solver grids), all in one sweep.  Row
        m = 0 and column n = 0 are exactly 1; out[..., -1, -1] is ``compute_Gram(X, Y)``.  Forward only on a default object: no ``grad_fn``, and
        paths that require grad raise outside ``torch.no_grad()``; gradients under ``exact_gradient=True``, see below.  Batches of unequal length: pad every path at its end with anything and gather
        node (len_a - 1, len_b - 1).  ``max_batch`` is accepted and ignored, as elsewhere.

        ``nodes`` keeps a slice of every grid instead of the grid -- the same sweep, the same values bit for bit, but neither the
        stores nor the memory of batch_X x batch_Y x len_x x len_y elements:
          "diagonal"  (batch_X, batch_Y, min(len_x, len_y)):  out[a, b, t] = k(X^a[:t+1], Y^b[:t+1]), a kernel as a function of time
          "last_row"  (batch_X, batch_Y, len_y):              out[a, b, n] = k(X^a, Y^b[:n+1]), a stream Y^b against complete paths
          "last_col"  (batch_X, batch_Y, len_x):              out[a, b, m] = k(X^a[:m+1], Y^b)
        Element 0 is exactly 1; the last element of "last_row" / "last_col" (of "diagonal" when len_x == len_y) is ``compute_Gram(X, Y)``.
        Any other string raises ``ValueError``.

        Gradients: under ``SigKernel(..., exact_gradient=True)`` X and Y both receive the true gradient of any function of the returned
        values -- the same values, bit for bit, as the no-grad call -- for every ``nodes`` mode.  The solver is a linear recursion in
        K, so the backward of the whole grid, or of any slice or weighting of it, is ONE reverse sweep per pair with each node's
        upstream weight injected at that node: what a ``compute_Gram`` backward costs on such an object, not one backward per
        prefix.  ``nodes="diagonal"`` on paths of unequal length: the points beyond min(len_x, len_y) get exactly zero.  Where
        ``X is Y`` autograd adds the two contributions; fp32 paths get fp32 gradients of an fp64 backward; one-point paths get zeros."""
        return self._prefixes(X, Y, True, max_batch, nodes)

    def compute_kernel_prefixes(self, X, Y, max_batch=100, nodes="all"):
        """X (batch, len_x, dim), Y (batch, len_y, dim) -> (batch, len_x, len_y): the paired form of ``compute_Gram_prefixes``;
        out[..., -1, -1] is ``compute_kernel(X, Y)``.  ``nodes``: as there, without the batch_Y axis.  Gradients: as there -- under
        ``exact_gradient=True``, for both arguments, one reverse sweep per pair."""
        return self._prefixes(X, Y, False, max_batch, nodes)

    def compute_mmd_prefixes(self, X, Y, max_batch=100):
        """X (batch_X, len_x, dim), Y (batch_Y, len_y, dim) -> (min(len_x, len_y),): value t is ``compute_mmd(X[:, :t+1], Y[:, :t+1])``
        -- the unbiased MMD^2 of the two samples as a function of time (sequential two-sample tests, change detection) -- from three
        ``nodes="diagonal"`` sweeps (K_XX, K_YY, K_XY) and the reductions of ``compute_mmd`` over the pair axes; value 0 is 0 (every
        kernel of one-point paths is 1); nothing of size pairs x len_x x len_y is allocated by the forward.  Forward only on a default
        object; under ``exact_gradient=True`` a composition of three differentiable ``nodes="diagonal"`` calls, so that a loss over time
        ``sum_t w_t MMD^2_t`` trains X and Y with three backward sweeps in all, not three per t."""
        if _wants_grad(X, Y) and not self.exact_gradient:
            raise NotImplementedError("compute_mmd_prefixes is forward only on this object: the reference's adjoint formula has no "
                                      "prefix form.  Construct the SigKernel with exact_gradient=True for its true gradient, or call "
                                      "it under torch.no_grad() or on detached paths")
        T = min(X.shape[1], Y.shape[1])
        K_XX = self.compute_Gram_prefixes(X, X, max_batch, nodes="diagonal")[..., :T]
        K_YY = self.compute_Gram_prefixes(Y, Y, max_batch, nodes="diagonal")[..., :T]
        K_XY = self.compute_Gram_prefixes(X, Y, max_batch, nodes="diagonal")
        A, B = K_XX.shape[0], K_YY.shape[0]
        # compute_mmd's estimator per t: the means of K_XX and K_YY without their diagonals (pairs a != a'), minus twice the mean of K_XY
        K_XX_m = (torch.sum(K_XX, dim=(0, 1)) - torch.sum(torch.diagonal(K_XX, dim1=0, dim2=1), dim=-1)) / (A * (A - 1.))
        K_YY_m = (torch.sum(K_YY, dim=(0, 1)) - torch.sum(torch.diagonal(K_YY, dim1=0, dim2=1), dim=-1)) / (B * (B - 1.))
        return K_XX_m + K_YY_m - 2. * torch.mean(K_XY, dim=(0, 1))

    def _ragged(self, X, Y, len_x, len_y, gram, what):
        f = self._on_features()
        if f is not None:
            return f[0]._ragged(f[1](X), f[1](Y), len_x, len_y, gram, what)
        _check_inputs(X, Y, paired=not gram)
        if self.process_group is not None:
            raise NotImplementedError("%s is not sharded over a process group; call it on a SigKernel without process_group" % what)
        if _wants_grad(X, Y) and not self.exact_gradient:
            raise NotImplementedError("%s is forward only on this object: the reference's adjoint formula is not built for ragged "
                                      "batches.  Construct the SigKernel with exact_gradient=True for their true gradient, or call it "
                                      "under torch.no_grad() or on detached paths" % what)
        lx = _lengths("len_x", len_x, X.shape[0], X.shape[1], X.device)
        ly = _lengths("len_y", len_y, Y.shape[0], Y.shape[1], Y.device)
        params = self._params()
        if _wants_grad(X, Y, *params):
            return _SigKernelRaggedExact.apply(X, Y, lx, ly, self.static_kernel, self.dyadic_order, gram, self._naive_solver,
                                               self.workspace_bytes, *params)
        return _prefix_at(_lib.get_backend(), self.static_kernel, X.detach(), Y.detach(), lx, ly, self.dyadic_order, self._naive_solver,
                          gram, self.workspace_bytes)

    def compute_Gram_ragged(self, X, Y, len_x, len_y, sym=False, max_batch=100):
        """Gram matrix of two batches of paths of UNEQUAL length: X (batch_X, Lx, dim), Y (batch_Y, Ly, dim) hold the paths padded at
        their ends to common lengths (``pad_paths``; any padding), len_x (batch_X,) / len_y (batch_Y,) their point counts ->
        (batch_X, batch_Y): out[a, b] = k(X^a[:len_x[a]], Y^b[:len_y[b]]) -- node (len_x[a] - 1, len_y[b] - 1) of
        ``compute_Gram_prefixes``'s grid, bit for bit: one sweep of the padded pairs by the fused prefix kernel that stores that one node
        per pair (dim <= 8, one band per pair; else increments in row tiles within ``workspace_bytes`` and a solver that again stores
        one node per pair and no grid -- by default every pair's own sub-grid, the same bits; ``routes.ragged_stream``: the streaming
        solver's padded sweep, within 1e-11 of them):
        the (batch_X, batch_Y, Lx, Ly) tensor is never built.  A path of one point gives exactly 1.  The values past a path's length
        never reach its result, whatever they are -- huge, NaN or inf (a function-valued static kernel maps them through its feature
        map first: keep them finite there).  The lengths are integer tensors (any device) or sequences of ints, checked once on the host: a wrong
        count, a non-integer dtype or a value outside [1, padded length] raises ``ValueError``.  ``sym=True`` requires ``Y is X`` and equal lengths; every pair is computed and the matrix then symmetrised
        (K + K^T) / 2.  A forward sweep costs what the PADDED shape costs: sort or bucket by length first where lengths vary a
        lot.  ``max_batch`` is accepted and ignored, as elsewhere.

        Gradients: forward only on a default object (paths that require grad raise ``NotImplementedError`` outside
        ``torch.no_grad()``).  Under ``SigKernel(..., exact_gradient=True)`` X and Y both receive the true gradient of the returned
        values -- the same values, bit for bit, as the no-grad call: the backward sweeps every pair over its OWN sub-grid (its cost
        follows the true lengths, not the padded ones) and runs the chain rule on the padded paths.  The padding may hold any
        values (NaN and inf included: the backward overwrites it with each path's last true point) and receives a gradient of exactly zero, as does a one-point path; where ``X is Y`` autograd adds the two
        contributions; fp32 paths get fp32 gradients of an fp64 backward."""
        if sym:
            if Y is not X:
                raise ValueError("sym=True needs Y is X")
            if len_y is not len_x and X.dim() >= 2:
                len_x = _Lengths("len_x", len_x, X.shape[0], X.shape[1], X.device)
                len_y = _Lengths("len_y", len_y, X.shape[0], X.shape[1], X.device)
                if not torch.equal(len_x.host, len_y.host):
                    raise ValueError("sym=True needs len_y equal to len_x")
        K = self._ragged(X, Y, len_x, len_y, True, "compute_Gram_ragged")
        return 0.5 * (K + K.transpose(0, 1)) if sym else K

    def compute_kernel_ragged(self, X, Y, len_x, len_y, max_batch=100):
        """The paired form of ``compute_Gram_ragged``: X (batch, Lx, dim), Y (batch, Ly, dim), len_x / len_y (batch,) -> (batch,):
        out[i] = k(X^i[:len_x[i]], Y^i[:len_y[i]]).  Gradients as there: under ``exact_gradient=True`` for both arguments, the padding
        (any values) receiving exactly zero; forward only on a default object."""
        return self._ragged(X, Y, len_x, len_y, False, "compute_kernel_ragged")

    def compute_mmd_ragged(self, X, len_x, Y, len_y, max_batch=100):
        """``compute_mmd``'s unbiased MMD^2 estimator on two samples of paths of unequal length (padded as for
        ``compute_Gram_ragged``): three ragged Gram matrices, K_XX and K_YY without their diagonals.  Forward only on a default object;
        under ``exact_gradient=True`` a composition of three ``compute_Gram_ragged`` calls with their true gradients, for X and Y (the
        padding -- any values -- receives exactly zero)."""
        if X.dim() >= 2 and Y.dim() >= 2:      # (a feature map keeps batch and length: axes 0 and 1)
            len_x = _Lengths("len_x", len_x, X.shape[0], X.shape[1], X.device)
            len_y = _Lengths("len_y", len_y, Y.shape[0], Y.shape[1], Y.device)
        K_XX = self.compute_Gram_ragged(X, X, len_x, len_x, sym=True, max_batch=max_batch)
        K_YY = self.compute_Gram_ragged(Y, Y, len_y, len_y, sym=True, max_batch=max_batch)
        K_XY = self.compute_Gram_ragged(X, Y, len_x, len_y, sym=False, max_batch=max_batch)
        K_XX_m = (torch.sum(K_XX) - torch.sum(torch.diag(K_XX))) / (K_XX.shape[0] * (K_XX.shape[0] - 1.))
        K_YY_m = (torch.sum(K_YY) - torch.sum(torch.diag(K_YY))) / (K_YY.shape[0] * (K_YY.shape[0] - 1.))
        return K_XX_m + K_YY_m - 2. * torch.mean(K_XY)

    def compute_kernel_and_derivatives_Gram(self, X, Y, gamma, max_batch=100):
        """X (batch_X, len_x, dim), Y (batch_Y, len_y, dim), gamma (batch_X, len_x, dim) -> three (batch_X, batch_Y)
        matrices: k(X^i, Y^j) and its first and second directional derivative along gamma^i (sigkernel.py:43-89)."""
        if self.process_group is not None:
            from .distributed import sharded_kgrad
            return sharded_kgrad(self, X, Y, gamma, self.process_group)
        return k_kgrad(X, Y, gamma, self.dyadic_order, self.static_kernel, workspace_bytes=self.workspace_bytes)

    def compute_Gram(self, X, Y, sym=False, max_batch=100):
        """X (batch_X, len_x, dim), Y (batch_Y, len_y, dim) -> (batch_X, batch_Y) matrix k(X^i_T, Y^j_T)."""
        f = self._on_features()
        if f is not None:
            return f[0].compute_Gram(f[1](X), f[1](Y), sym, max_batch)
        if self.process_group is not None:
            from .distributed import sharded_gram
            return sharded_gram(self, X, Y, sym, self.process_group)
        params = self._params()
        if not _wants_grad(X, Y, *params):
            return _SigKernelGram.forward(_NoGradCtx(), X, Y, self.static_kernel, self.dyadic_order, sym, self._naive_solver,
                                          self.workspace_bytes)
        if self.exact_gradient:
            return _SigKernelExact.apply(X, Y, self.static_kernel, self.dyadic_order, True, sym, self._naive_solver, self.workspace_bytes,
                                         *params)
        return _SigKernelGram.apply(X, Y, self.static_kernel, self.dyadic_order, sym, self._naive_solver,
                                    self.workspace_bytes)

    def compute_distance(self, X, Y, max_batch=100):
        """(batch,) paired squared distances reduced to their mean, as the reference does (sigkernel.py:130-144)."""
        assert self.exact_gradient or not Y.requires_grad, "the second input should not require grad"
        f = self._on_features()
        if f is not None:
            return f[0].compute_distance(f[1](X), f[1](Y), max_batch)
        n = X.shape[0] if X.dim() == 3 else 0
        if (not self.exact_gradient and not routes.no_merged_loss and X.dim() == 3 and X.shape == Y.shape and X.dtype == Y.dtype and X.device == Y.device and n > 0
                and X.shape[1] >= 2 and float(n) * float((X.shape[1] - 1) << int(self.dyadic_order)) ** 2 < _cost("paired_merge_cells")):
            # training-sized batches: k(x_i, x_i) and k(x_i, y_i) as ONE paired batch of 2n pairs -- one forward and one adjoint launch
            # instead of two each (launch- and fill-bound at these sizes); the same per-pair values, and the gradient reaches X through
            # the first argument of both halves, as in the reference's three calls (_SigKernel returns none for a second argument)
            K2 = self.compute_kernel(torch.cat((X, X)), torch.cat((X.detach(), Y)), max_batch)
            K_YY = self.compute_kernel(Y, Y, max_batch)
            return torch.mean(K2[:n]) + torch.mean(K_YY) - 2. * torch.mean(K2[n:])
        K_XX = self.compute_kernel(X, X, max_batch)
        K_YY = self.compute_kernel(Y, Y, max_batch)
        K_XY = self.compute_kernel(X, Y, max_batch)
        return torch.mean(K_XX) + torch.mean(K_YY) - 2. * torch.mean(K_XY)

    def compute_scoring_rule(self, X, y, max_batch=100):
        """S(X, y) = E[k(X, X)] - 2 E[k(X, y)] with y of shape (1, len_y, dim) (sigkernel.py:146-161)."""
        assert self.exact_gradient or not y.requires_grad, "the second input should not require grad"
        f = self._on_features()
        if f is not None:
            return f[0].compute_scoring_rule(f[1](X), f[1](y), max_batch)
        merged = self._merged_loss(X, y, with_yy=False)
        if merged is not None:
            return merged
        K_XX = self.compute_Gram(X, X, sym=True, max_batch=max_batch)
        K_Xy = self.compute_Gram(X, y, sym=False, max_batch=max_batch)
        K_XX_m = (torch.sum(K_XX) - torch.sum(torch.diag(K_XX))) / (K_XX.shape[0] * (K_XX.shape[0] - 1.))
        return K_XX_m - 2. * torch.mean(K_Xy)

    def compute_expected_scoring_rule(self, X, Y, max_batch=100):
        """S(X, Y) = E_Y[S(X, y)] (sigkernel.py:163-178)."""
        assert self.exact_gradient or not Y.requires_grad, "the second input should not require grad"
        f = self._on_features()
        if f is not None:
            return f[0].compute_expected_scoring_rule(f[1](X), f[1](Y), max_batch)
        merged = self._merged_loss(X, Y, with_yy=False)
        if merged is not None:
            return merged
        K_XX = self.compute_Gram(X, X, sym=True, max_batch=max_batch)
        K_XY = self.compute_Gram(X, Y, sym=False, max_batch=max_batch)
        K_XX_m = (torch.sum(K_XX) - torch.sum(torch.diag(K_XX))) / (K_XX.shape[0] * (K_XX.shape[0] - 1.))
        return K_XX_m - 2. * torch.mean(K_XY)

    def _merged_loss(self, X, Y, with_yy):
        """The loss wrappers' merged route for training-sized batches (_SigKernelLoss: one forward and one adjoint launch over
        K(X, [X; Y])), or None where it does not apply -- paths of different lengths, a process group, batches whose K_XX the
        composition solves as a blocked triangle (_SYM_MIN_CELLS grid cells and more: that saves more than the merged launches
        do; below it, measured on one box from 16 to 512 paths, tools/experiments/r04_merged_loss.py: merged 0.30 / 0.31 / 0.56 /
        1.27 / 4.16 / 15.1 ms against 0.58 / 0.58 / 0.80 / 1.57 / 4.48 / 15.5 at 16 / 32 / 64 / 128 / 256 / 512 paths of
        BASELINE configs[1]'s shape), fewer than two paths (the reference's 0 / 0), malformed inputs (the Gram calls raise for
        those), `routes.no_merged_loss`."""
        if self.exact_gradient or routes.no_merged_loss or self.process_group is not None or X.dim() != 3 or Y.dim() != 3:
            return None      # (exact_gradient: the loss is a composition of compute_Gram calls, each with its true gradient)
        A, B = X.shape[0], Y.shape[0]
        if X.shape[1:] != Y.shape[1:] or X.shape[1] < 2 or A < 2 or B < (2 if with_yy else 1) or X.dtype != Y.dtype or X.device != Y.device:
            return None
        if float(A) * A * float((X.shape[1] - 1) << int(self.dyadic_order)) ** 2 >= _cost("sym_min_cells"):
            return None
        args = (X, Y, self.static_kernel, self.dyadic_order, self._naive_solver, self.workspace_bytes, with_yy)
        if not _wants_grad(X):
            return _SigKernelLoss.forward(_NoGradCtx(), *args)
        return _SigKernelLoss.apply(*args)

    def compute_mmd(self, X, Y, max_batch=100):
        """Unbiased MMD^2 between the samples X and Y (sigkernel.py:180-197).

        Training-sized batches (a few thousand pairs per Gram matrix) leave most of the chip idle: each of the three forward
        launches -- and, in backward, of the two adjoint launches -- is a wave's skew fill plus a pair or two.  While a hipGraph is
        being CAPTURED (`torch.cuda.graph`: what a training loop with static shapes should replay) the three Gram matrices are
        therefore put on three streams -- K_YY and K_XY fork from the caller's stream and join it before the reductions; autograd
        runs each matrix's backward on the stream of its forward -- so the graph holds them as parallel branches: replays 10-15 %
        faster at 16..64 paths (tools/experiments/r04_mmd_streams.py), bit-identical gradients.  Eager calls stay on one stream:
        they are bound by the host's launch rate there, and the stream switches cost more than the overlap returns (0.59 -> 0.75 ms
        at 32 paths); large batches fill the chip with one launch (round 3: no gain from streams at BASELINE configs[3])."""
        assert self.exact_gradient or not Y.requires_grad, "the second input should not require grad"
        f = self._on_features()
        if f is not None:
            return f[0].compute_mmd(f[1](X), f[1](Y), max_batch)
        merged = self._merged_loss(X, Y, with_yy=True)
        if merged is not None:
            return merged
        small = (X.is_cuda and Y.is_cuda and self.process_group is None and routes_allow_streams()
                 and max(X.shape[0], Y.shape[0]) ** 2 <= _cost("mmd_streams_max_pairs") and X.shape[0] > 1 and Y.shape[0] > 1)
        if small:
            s_yy, s_xy = _side_streams(X.device)      # (created by the warm-up calls that precede a capture, never inside one)
        if small and torch.cuda.is_current_stream_capturing():
            cur = torch.cuda.current_stream(X.device)
            s_yy.wait_stream(cur)
            s_xy.wait_stream(cur)
            with torch.cuda.stream(s_yy):
                K_YY = self.compute_Gram(Y, Y, sym=True, max_batch=max_batch)
            with torch.cuda.stream(s_xy):
                K_XY = self.compute_Gram(X, Y, sym=False, max_batch=max_batch)
            K_XX = self.compute_Gram(X, X, sym=True, max_batch=max_batch)
            cur.wait_stream(s_yy)
            cur.wait_stream(s_xy)
            K_YY.record_stream(cur)       # (allocated on the side streams, consumed on the caller's)
            K_XY.record_stream(cur)
        else:
            K_XX = self.compute_Gram(X, X, sym=True, max_batch=max_batch)
            K_YY = self.compute_Gram(Y, Y, sym=True, max_batch=max_batch)
            K_XY = self.compute_Gram(X, Y, sym=False, max_batch=max_batch)
        K_XX_m = (torch.sum(K_XX) - torch.sum(torch.diag(K_XX))) / (K_XX.shape[0] * (K_XX.shape[0] - 1.))
        K_YY_m = (torch.sum(K_YY) - torch.sum(torch.diag(K_YY))) / (K_YY.shape[0] * (K_YY.shape[0] - 1.))
        return K_XX_m + K_YY_m - 2. * torch.mean(K_XY)
