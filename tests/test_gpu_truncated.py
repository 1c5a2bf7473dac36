"""truncated_sig_kernel on the GPU: the public function on the HIP route (k_trunc_sig, csrc/sk_truncated.hip) against the reference's
recorded outputs (tests/golden/truncated.npz) and against the torch restatement of the recursion on a sweep of lengths, dims, levels,
orders and batch sizes; the launch trace (sk_launch_trace) proves which route ran.

Bars: fp64 <= 1e-12 of the matrix's max-norm; fp32 I/O rtol 1e-4 / atol 1e-5.  Steps are scaled to norm 0.2-0.5 so
that level 8 neither vanishes nor dominates."""
import numpy as np
import pytest
import torch

from test_truncated_host import assert_close, fixtures, sigma_arg, steps

pytestmark = pytest.mark.gpu

ORDER1, GENERAL = "k_trunc_sigILi1ELi2E", "k_trunc_sigILi4ELi1E"


def traced(fn):
    """fn() with the library counting its launches: (result, {instance tag: launches} of k_trunc_sig)"""
    from sigkernel_amd import _lib
    was = _lib.launch_trace(True)
    try:
        _lib.launch_counts(reset=True)
        out = fn()
        torch.cuda.synchronize()
        counts = _lib.launch_counts()
    finally:
        _lib.launch_trace(was)
    hit = {}
    for name, n in counts.items():
        for tag in (ORDER1, GENERAL):
            if tag in name and n > 0:
                hit[tag] = hit.get(tag, 0) + n
    return out, hit


def expected_instance(L, order):
    return ORDER1 if min(L, L if order < 1 else order) == 1 else GENERAL


def expected_launches(L, order):
    """the kernel is built for orders <= 4: a full-order call of five or six levels takes the torch route"""
    return {} if min(L, L if order < 1 else order) > 4 else {expected_instance(L, order): 1}


@pytest.mark.parametrize("case", range(17))
def test_hip_route_reproduces_the_reference(case):
    import sigkernel_amd
    c, X, Y, L, sigma, order, K = list(fixtures())[case]
    Xd, Yd = torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda()
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xd, Yd, L, sigma=sigma_arg(sigma), order=order))
    assert hit == expected_launches(L, order), hit                # (steps <= 12, dim <= 12, levels <= 6: only the order decides the route)
    assert got.shape == K.shape and got.dtype == Xd.dtype and got.is_cuda
    assert_close(got.cpu().numpy(), K, X.dtype.type, c)
    # the torch route on the device, and numpy in / numpy out (the reference's own call)
    from sigkernel_amd.truncated import _truncated_torch
    assert_close(_truncated_torch(Xd, Yd, L, sigma_arg(sigma), order).cpu().numpy(), K, X.dtype.type, (c, "torch"))
    Kn = sigkernel_amd.transforms.truncated_sig_kernel(X, Y, L, sigma=sigma, order=order)
    assert isinstance(Kn, np.ndarray) and Kn.dtype == X.dtype
    assert np.array_equal(Kn, got.cpu().numpy())


# (A, B, M, N, D, L, order): rows 2, 3, 63-66, 127-130; odd N; dims 1-16; levels 1-8; every built order; batches around the number of
# resident single-wave workgroups (8 per CU, 2048 on 256 CUs: one position each, then a second round for some) and lane groups with
# idle members (A not a multiple of the groups per wave)
SWEEP = [(3, 4, 2, 3, 1, 1, -1), (3, 4, 3, 5, 2, 2, -1), (5, 3, 2, 7, 3, 8, 1), (5, 7, 3, 9, 16, 8, 4), (9, 2, 8, 11, 9, 3, 3),
         (3, 4, 63, 33, 4, 8, 4), (3, 4, 64, 65, 8, 8, 4), (3, 4, 64, 127, 16, 8, 3), (3, 4, 63, 129, 5, 7, 2), (2, 3, 64, 255, 7, 5, 2),
         (3, 4, 63, 65, 6, 8, 1), (3, 4, 64, 63, 7, 4, 1), (3, 4, 65, 67, 8, 8, 1), (3, 4, 66, 31, 10, 6, 1), (3, 4, 127, 129, 4, 8, 1),
         (3, 4, 128, 127, 16, 8, 1), (2, 3, 128, 255, 8, 8, 1), (4, 3, 33, 17, 12, 1, -1), (4, 3, 17, 33, 13, 2, 2), (4, 3, 40, 21, 15, 3, 3),
         (4, 3, 40, 21, 11, 4, -1), (4, 3, 30, 19, 14, 4, 1), (3, 5, 16, 127, 16, 6, 4),
         (32, 64, 40, 9, 3, 4, 2), (23, 89, 40, 9, 3, 4, 1), (41, 50, 40, 9, 3, 5, 3), (2049, 1, 70, 5, 2, 3, 1), (1, 2049, 33, 5, 2, 3, 3),
         (130, 33, 8, 7, 4, 6, 4)]
# the same kernel on (y, x): only the second batch fits the lanes
SWAPPED = [(3, 4, 65, 63, 8, 8, 4), (3, 4, 66, 33, 5, 6, 2), (3, 4, 129, 127, 4, 8, 1), (3, 4, 130, 65, 8, 5, 1), (2, 3, 200, 21, 3, 4, 3)]
# outside the kernel's scope either way: the torch route, no launch of k_trunc_sig
OUTSIDE = [(3, 4, 65, 65, 8, 8, 4), (3, 4, 129, 129, 4, 8, 1), (3, 4, 130, 131, 4, 3, 1), (2, 3, 127, 129, 4, 8, 2), (3, 4, 20, 15, 17, 3, 1),
           (3, 4, 20, 15, 4, 9, 1), (3, 4, 20, 15, 4, 6, 5), (2, 2, 64, 257, 8, 3, 2), (2, 2, 64, 129, 9, 3, 2)]


def run_case(A, B, M, N, D, L, order, dtype, seed):
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(seed)
    X, Y = torch.as_tensor(steps(rng, A, M, D, dtype)).cuda(), torch.as_tensor(steps(rng, B, N, D, dtype)).cuda()
    sigma = torch.as_tensor(rng.uniform(0.5, 1.5, L + 1).astype(dtype))
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=sigma, order=order))
    want = _truncated_torch(X.double(), Y.double(), L, sigma.double(), order)
    err = float((got.double() - want).abs().max() / want.abs().max())
    print("truncated %s A %d B %d M %d N %d D %d L %d order %d: max-norm error %.3g, launches %s" % (np.dtype(dtype).name, A, B, M, N, D, L, order, err, hit))
    assert got.shape == (A, B) and got.dtype == X.dtype
    assert_close(got.cpu().numpy(), want.cpu().numpy(), dtype, (A, B, M, N, D, L, order))
    return hit


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("shape", SWEEP + SWAPPED)
def test_hip_route_against_the_torch_route(shape, dtype):
    A, B, M, N, D, L, order = shape
    hit = run_case(A, B, M, N, D, L, order, dtype, 1000 + M + 7 * N)
    assert hit == {expected_instance(L, order): 1}, hit


@pytest.mark.parametrize("shape", OUTSIDE)
def test_shapes_outside_the_kernel_take_the_torch_route(shape):
    """The ROUTE is what this checks (no launch of k_trunc_sig): the public function runs the torch restatement here, so the comparison in
    run_case is that route with itself.  Its VALUES are held to the reference by the order-5 / order-6 fixtures of
    test_hip_route_reproduces_the_reference and, below, to Chen's identity on shapes no fixture has."""
    A, B, M, N, D, L, order = shape
    assert run_case(A, B, M, N, D, L, order, np.float64, 5) == {}


@pytest.mark.parametrize("A,B,M,N,D,L", [(2, 2, 6, 5, 17, 3), (2, 2, 5, 4, 2, 9), (1, 2, 66, 65, 2, 5)])
def test_out_of_scope_values_against_chens_identity(A, B, M, N, D, L):
    """full order outside the kernel (dim 17; nine levels; five levels on 66 x 65 steps): the public function against the tensor levels"""
    import sigkernel_amd
    from test_truncated_host import chen_kernel
    rng = np.random.default_rng(17 + M)
    X, Y = steps(rng, A, M, D), steps(rng, B, N, D)
    sigma = rng.uniform(0.5, 1.5, L + 1)
    got, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(torch.as_tensor(X).cuda(), torch.as_tensor(Y).cuda(), L, sigma=torch.as_tensor(sigma)))
    assert hit == {}
    assert_close(got.cpu().numpy(), chen_kernel(X, Y, L, sigma), np.float64, (M, N, D, L))


def test_backend_entry_point_states_its_scope():
    """HipBackend.truncated_gram: the matrix inside sk_route_query(SK_OP_TRUNCATED) == FUSED, None outside (the caller then tries (y, x))"""
    from sigkernel_amd import _lib
    from sigkernel_amd.truncated import _truncated_torch
    be = _lib.get_backend()
    rng = np.random.default_rng(4)
    X, Y = torch.as_tensor(steps(rng, 3, 70, 4)).cuda(), torch.as_tensor(steps(rng, 2, 30, 4)).cuda()
    w = [1.0, 0.5, 2.0, 0.25]
    assert be.truncated_gram(X, Y, 3, w, 2) is None                         # 70 rows at order 2: only (y, x) fits
    Kt = be.truncated_gram(Y, X, 3, w, 2)
    assert_close(Kt.t().cpu().numpy(), _truncated_torch(X, Y, 3, w, 2).cpu().numpy(), np.float64)
    assert_close(be.truncated_gram(X, Y, 3, w, 1).cpu().numpy(), _truncated_torch(X, Y, 3, w, 1).cpu().numpy(), np.float64)


def test_inputs_that_require_grad_take_the_differentiable_route():
    import sigkernel_amd
    from sigkernel_amd.truncated import _truncated_torch
    rng = np.random.default_rng(11)
    Xc, Yc = torch.as_tensor(steps(rng, 2, 4, 2)), torch.as_tensor(steps(rng, 2, 3, 2))
    sig = torch.as_tensor(rng.uniform(0.5, 1.5, 5))
    w = torch.as_tensor(rng.standard_normal((2, 2)))
    for order in (-1, 1, 2):
        Xh, Yh = Xc.clone().requires_grad_(), Yc.clone().requires_grad_()
        (_truncated_torch(Xh, Yh, 4, sig, order) * w).sum().backward()
        Xg, Yg = Xc.cuda().requires_grad_(), Yc.cuda().requires_grad_()
        K, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xg, Yg, 4, sigma=sig, order=order))
        assert hit == {} and K.requires_grad
        (K * w.cuda()).sum().backward()
        assert_close(Xg.grad.cpu().numpy(), Xh.grad.numpy(), np.float64, ("dX", order))
        assert_close(Yg.grad.cpu().numpy(), Yh.grad.numpy(), np.float64, ("dY", order))
        # without a gradient pending the same tensors go through the kernel
        with torch.no_grad():
            _, hit = traced(lambda: sigkernel_amd.truncated_sig_kernel(Xg, Yg, 4, sigma=sig, order=order))
        assert sum(hit.values()) == 1


@pytest.mark.parametrize("shape", [(37, 29, 64, 65, 8, 8, 4), (37, 29, 128, 65, 8, 8, 1), (300, 9, 20, 33, 3, 6, 2)])
def test_repeated_calls_are_bitwise_identical(shape):
    import sigkernel_amd
    A, B, M, N, D, L, order = shape
    rng = np.random.default_rng(2)
    X, Y = torch.as_tensor(steps(rng, A, M, D)).cuda(), torch.as_tensor(steps(rng, B, N, D)).cuda()
    first = sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=0.9, order=order)
    for _ in range(4):
        assert torch.equal(sigkernel_amd.truncated_sig_kernel(X, Y, L, sigma=0.9, order=order), first)
