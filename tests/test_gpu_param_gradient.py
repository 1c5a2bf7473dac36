"""SigKernel(exact_gradient=True) with a learnable RBFKernel.sigma, on the GPU: k_static_rbf_adj's parameter mode (one launch gives dL/dX
and dL/dsigma) against CPU fp64 torch autograd through the restatement (tests/param_gradient_reference.py), gradcheck over (X, Y, sigma)
through the public methods, the bits the mode must not move, and the C entry point's refusals.

The bar for the scalar sigma.grad: |got - want| <= 1e-9 x sum over pairs of |go_p dK_p / d sigma| -- the project's gradient bar scaled by
the pairs' own terms, so that cancellation in the sum can neither hide nor fake an error.  Every test prints its measured ratio first."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sigkernel_amd
from sigkernel_amd import _lib
from poison import poisoned, same_bits
import param_gradient_reference as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRADCHECK = dict(eps=1e-6, atol=1e-7, rtol=1e-6)      # the bar of the project's gradcheck tests
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_gradient_parent.npz")
GOLDEN_CASES = ("d2", "d11", "d11_paired", "d20")
# the sites whose integer allocations tests/test_gpu_poison.py has audited (initialised on the launch stream before their first read)
AUDITED = frozenset(("_lib", f) for f in ("_queue", "solve_fwd_fused_static", "linear_adjoint_fused_mb", "rbf_adjoint_fused_mb", "solve_deriv_fused",
                                          "_fused_rescue_args", "solve_adj", "_grid_scratch"))

# what each shape of P.CASES can break, and the kernel instance it must reach (None: the generic branch, no parameter-mode launch)
#   d2   <4, 64, RM 4>: M = 6 is no multiple of RM (clamped and masked rows), B = 3 leaves an odd tail to the two-pairs-in-flight loop
#   d7   <8, 64>: N = 70 > NT, the strided column loop
#   d11  <16, 128, RM 2>, as a Gram block and paired (B = 0)
#   d20  <24, 128, RM 1>: N = 6 -- a float-sigma call runs the tiled kernel here, the parameter mode leaves it
#   d32  DMAX 32 with N = 130 > 128
#   d40  beyond the fused static kernels: the generic branch
INSTANCE = {"d2": "k_static_rbf_adjIdLi4ELi64ELi4E", "d2_naive": "k_static_rbf_adjIdLi4ELi64ELi4E", "d7": "k_static_rbf_adjIdLi8ELi64ELi4E",
            "d11": "k_static_rbf_adjIdLi16ELi128ELi2E", "d11_paired": "k_static_rbf_adjIdLi16ELi128ELi2E",
            "d20": "k_static_rbf_adjIdLi24ELi128ELi1E", "d32": "k_static_rbf_adjIdLi32ELi128ELi1E", "d40": None}


def _sigma(value, dtype=torch.float64):
    return torch.tensor(value, dtype=dtype, device=DEV, requires_grad=True)


def _run(name, sigma, need_paths=True, dtype=torch.float64):
    """backward of sum(go * K) of a case on the device -> (X.grad, Y.grad, sigma.grad) (None where not asked for)"""
    D, A, B, M, N, d, naive = P.CASES[name]
    Xc, Yc, go, _ = P.case_inputs(name)
    X, Y = Xc.to(DEV, dtype).requires_grad_(need_paths), Yc.to(DEV, dtype).requires_grad_(need_paths)
    sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(sigma), d, _naive_solver=naive, exact_gradient=True)
    K = sk.compute_Gram(X, Y) if B else sk.compute_kernel(X, Y)
    (K * go.to(DEV, dtype)).sum().backward()
    return X.grad, Y.grad, (sigma.grad if isinstance(sigma, torch.Tensor) else None)


def _adj_launches(call):
    """(result, {k_static_rbf_adj* instance: launches}) of call()"""
    was = _lib.launch_trace(True)
    _lib.launch_counts(reset=True)
    try:
        out = call()
        torch.cuda.synchronize()
        counts = _lib.launch_counts(reset=True)
    finally:
        _lib.launch_trace(was)
    return out, {k.split(".kd")[0]: v for k, v in counts.items() if "k_static_rbf_adj" in k and v > 0}


@pytest.mark.parametrize("name", sorted(P.CASES))
def test_sigma_gradient_against_autograd(name):
    """X, Y and sigma all require grad: sigma.grad within the bar, from ONE launch of the instance the shape is chosen for (no tiled
    launch beside it); d40: the generic branch, no launch of the kernel at all"""
    _, _, _, sigma = P.case_inputs(name)
    s = _sigma(sigma)
    (gx, gy, gs), hit = _adj_launches(lambda: _run(name, s))
    want, scale = P.case_reference(name)
    err = abs(float(gs) - want)
    print("%s: sigma.grad %.15g, reference %.15g, |error| / sum_p |go_p dK_p/dsigma| = %.3e" % (name, float(gs), want, err / scale))
    assert gs.shape == s.shape and gs.dtype == torch.float64 and gs.device == s.device
    assert err <= P.GRAD_BAR * scale
    if INSTANCE[name] is None:
        assert not hit, hit
    else:
        B = P.CASES[name][2]
        mine = {k: v for k, v in hit.items() if INSTANCE[name] in k}
        # one launch for (dX, dsigma); a paired batch, and no other, has its dY from the same kernel on the swapped pairs (mode off)
        assert sum(mine.values()) == 1 and sum(hit.values()) == (1 if B else 2) and not any("tiled" in k for k in hit), hit


@pytest.mark.parametrize("name", ["d2", "d11_paired", "d20", "d40"])
def test_only_sigma_requires_grad(name):
    """sigma the only tensor that requires grad: backward works, the paths get nothing, and sigma.grad has the bits of the call where
    the paths require grad too (D <= 32: the same launch) -- within the bar either way"""
    _, _, _, sigma = P.case_inputs(name)
    s = _sigma(sigma)
    gx, gy, gs = _run(name, s, need_paths=False)
    assert gx is None and gy is None and gs is not None
    want, scale = P.case_reference(name)
    err = abs(float(gs) - want)
    print("%s, sigma alone: |error| / sum_p |terms| = %.3e" % (name, err / scale))
    assert err <= P.GRAD_BAR * scale
    if INSTANCE[name] is not None:
        s2 = _sigma(sigma)
        assert same_bits(gs, _run(name, s2)[2])[0]


def _gradcheck(fn, *inputs):
    assert torch.autograd.gradcheck(fn, inputs, **GRADCHECK)


def _small(seed, batch, length, dim=2):
    return P.walks(seed, batch, length, dim).to(DEV).requires_grad_(True)


@pytest.mark.parametrize("d", [0, 1])
def test_gradcheck_of_the_dense_calls(d):
    """A = 2, B = 3, M = 4, N = 5, D = 2 over (X, Y, sigma): compute_Gram, compute_kernel, compute_Gram(x, x, sym=True), compute_mmd"""
    X, Y, s = _small(1, 2, 4), _small(2, 3, 5), _sigma(0.7)
    Yp = _small(3, 2, 5)

    def sk(sig):
        return sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(sig), d, exact_gradient=True)
    _gradcheck(lambda x, y, sig: sk(sig).compute_Gram(x, y), X, Y, s)
    _gradcheck(lambda x, y, sig: sk(sig).compute_kernel(x, y), X, Yp, s)
    _gradcheck(lambda x, sig: sk(sig).compute_Gram(x, x, sym=True), X, s)
    _gradcheck(lambda x, y, sig: sk(sig).compute_mmd(x, y), X, Y, s)


def test_gradcheck_of_the_ragged_call():
    X, Y, s = _small(1, 2, 4), _small(2, 3, 5), _sigma(0.7)
    _gradcheck(lambda x, y, sig: sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(sig), 1, exact_gradient=True)
               .compute_Gram_ragged(x, y, [4, 2], [5, 3, 2]), X, Y, s)


@pytest.mark.parametrize("nodes", ["all", "diagonal", "last_row", "last_col"])
def test_gradcheck_of_the_prefix_calls(nodes):
    X, Y, s = _small(1, 2, 4), _small(2, 3, 5), _sigma(0.7)
    _gradcheck(lambda x, y, sig: sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(sig), 1, exact_gradient=True)
               .compute_Gram_prefixes(x, y, nodes=nodes), X, Y, s)


def test_gradcheck_of_a_function_valued_kernel():
    """RBF_ID_Kernel(sigma) on (batch, T, 2, 1) paths: its base kernel hands the tensor sigma on"""
    X = P.walks(5, 2, 4, 2).reshape(2, 4, 2, 1).to(DEV).requires_grad_(True)
    Y = P.walks(6, 3, 5, 2).reshape(3, 5, 2, 1).to(DEV).requires_grad_(True)
    _gradcheck(lambda x, y, sig: sigkernel_amd.SigKernel(sigkernel_amd.RBF_ID_Kernel(sig), 1, exact_gradient=True).compute_Gram(x, y),
               X, Y, _sigma(0.7))


def test_module_static_kernel_on_the_device():
    """a torch.nn.Module static kernel: the generic branch, its parameter's gradient against autograd through the restatement"""
    k = P.LearnableCubic().to(DEV)
    Xc, Yc = 0.5 * P.walks(21, 2, 4, 2), 0.5 * P.walks(22, 3, 5, 2)
    go = torch.randn(2, 3, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    sk = sigkernel_amd.SigKernel(k, 1, exact_gradient=True)
    (sk.compute_Gram(Xc.to(DEV), Yc.to(DEV)) * go.to(DEV)).sum().backward()
    ref = P.LearnableCubic()
    (want, scale), _ = P.per_pair_gradients(P.R.gram_torch(Xc, Yc, ref, 1), go, 2, (ref.c, ref.unused))
    err = abs(float(k.c.grad) - float(want))
    print("module coefficient: |error| / sum_p |terms| = %.3e" % (err / scale))
    assert err <= P.GRAD_BAR * scale and k.unused.grad.shape == (2,) and not k.unused.grad.any()


@pytest.mark.parametrize("name", ["d2", "d7", "d11", "d11_paired", "d20"])
def test_the_mode_keeps_the_bits_of_the_paths_gradients(name):
    """two identical calls: identical sigma.grad bits.  X.grad / Y.grad with sigma pending against the same call with float(sigma): bit
    for bit up to 16 dims (the same kernel instance, mode on and off); at 20 dims the float call runs the tiled kernel -- two routes of
    one quantity, 1e-12 x max as in test_tiled_backward_equals_the_untiled_one"""
    D = P.CASES[name][0]
    _, _, _, sigma = P.case_inputs(name)
    gx, gy, gs = _run(name, _sigma(sigma))
    gx2, gy2, gs2 = _run(name, _sigma(sigma))
    assert same_bits(gs, gs2)[0] and same_bits(gx, gx2)[0] and same_bits(gy, gy2)[0]
    fx, fy, _ = _run(name, sigma)
    for a, b, what in ((gx, fx, "X.grad"), (gy, fy, "Y.grad")):
        if D <= 16:
            ok, msg = same_bits(a, b)
            assert ok, "%s %s: %s" % (name, what, msg)
        else:
            gap = float((a - b).abs().max()) / float(b.abs().max())
            print("%s %s: parameter-mode route against the tiled route, %.3e x max" % (name, what, gap))
            assert gap <= 1e-12


def golden_inputs(name):
    """(X, Y, W, scale, sigma, gram) of a recorded static_adjoint call: the case's paths and weights and a random W, CPU fp64"""
    D, A, B, M, N, d, naive = P.CASES[name]
    X, Y, go, sigma = P.case_inputs(name)
    W = torch.randn(go.shape + (M - 1, N - 1), generator=torch.Generator().manual_seed(31 + D), dtype=torch.float64)
    return X, Y, W, go, sigma, B > 0


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_float_sigma_static_adjoint_returns_the_parents_bits(name):
    """sk_static_adjoint_f64 with the mode off: the bits recorded on the parent commit (tests/golden/make_golden_param_gradient_parent.py),
    and the parameter-mode launch's dX: the same bits where it is the same kernel instance (up to 16 dims)"""
    rec = np.load(GOLDEN)
    X, Y, W, go, sigma, gram = golden_inputs(name)
    for key, t in (("X", X), ("Y", Y), ("W", W), ("scale", go)):
        assert np.array_equal(rec[name + "/" + key], t.numpy()), "the inputs are not the recorded ones: " + key
    be = _lib.HipBackend()
    args = (1, sigma, X.to(DEV), Y.to(DEV), W.to(DEV), go.to(DEV), gram)
    got = be.static_adjoint(*args).cpu()
    want = torch.from_numpy(rec[name + "/dX"])
    ok, msg = same_bits(got, want)
    assert ok, msg
    dX, dparam = be.static_adjoint_param(*args)
    if P.CASES[name][0] <= 16:
        ok, msg = same_bits(dX.cpu(), want)
        assert ok, msg
    else:
        assert float((dX.cpu() - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert dparam.shape == () and dparam.dtype == torch.float64 and bool(torch.isfinite(dparam))


def test_poisoned_allocations_give_the_same_bits():
    """every torch.empty of the library filled with 0xFF (NaN) and 0x55 (huge, finite): the same sigma.grad, X.grad and Y.grad bits -- the
    partials behind dX are all written by the launch that is summed"""
    for name in ("d2", "d11_paired", "d20"):
        _, _, _, sigma = P.case_inputs(name)
        first = _run(name, _sigma(sigma))
        for byte in (0xFF, 0x55):
            with poisoned(byte, AUDITED) as p:
                out = _run(name, _sigma(sigma))
            torch.cuda.synchronize()
            assert p.count > 0 and p.sites.get(("_lib", "static_adjoint_param"), 0) >= 1, p.sites
            for a, b in zip(first, out):
                ok, msg = same_bits(a, b)
                assert ok, "%s under 0x%02X: %s" % (name, byte, msg)


def test_fp32_paths_and_sigma():
    """fp32 paths with an fp32 sigma: sigma.grad in fp32, equal to the fp64 object's on the same values at the project's fp32 bar"""
    name = "d2"
    _, _, _, sigma = P.case_inputs(name)
    s32 = _sigma(sigma, torch.float32)
    s64 = _sigma(float(s32.detach()))
    D, A, B, M, N, d, naive = P.CASES[name]
    Xc, Yc, go, _ = P.case_inputs(name)
    grads = []
    for dt, s in ((torch.float32, s32), (torch.float64, s64)):
        X, Y = Xc.float().to(DEV, dt).requires_grad_(True), Yc.float().to(DEV, dt).requires_grad_(True)
        sk = sigkernel_amd.SigKernel(sigkernel_amd.RBFKernel(s), d, exact_gradient=True)
        K = sk.compute_Gram(X, Y)
        assert K.dtype == dt
        (K * go.to(DEV, dt)).sum().backward()
        assert s.grad.dtype == dt and X.grad.dtype == dt
        grads.append(s.grad.double().cpu().numpy())
    np.testing.assert_allclose(grads[0], grads[1], rtol=1e-4, atol=1e-5)


def test_c_entry_refusals_and_the_partial_tail():
    """sk_static_adjoint_param_f64 itself on device buffers full of NaN: kind 0 and D = 33 are unsupported (2), a null partial pointer and a
    wrong partial count are bad arguments (1) -- refused by argument check: the buffers stay NaN -- and a valid call writes every element
    of dX and of the partial tail, the partials adding up to sigma^2 x the binding's dparam"""
    name = "d2"
    D, A, B, M, N, d, naive = P.CASES[name]
    X, Y, W, go, sigma, gram = golden_inputs(name)
    X, Y, W, go = X.to(DEV), Y.to(DEV), W.to(DEV), go.to(DEV)
    fn = _lib.load().sk_static_adjoint_param_f64
    need = ctypes.c_int64(0)
    assert fn(1, sigma, None, None, None, 0, None, A, B, M, N, D, None, None, ctypes.byref(need), None) == 0
    assert need.value == A * ((M + 3) // 4)
    buf = torch.full((A * M * D + need.value + 4,), float("nan"), dtype=torch.float64, device=DEV)
    tail = buf.data_ptr() + 8 * A * M * D

    def call(kind=1, dim=D, partials=tail, count=need.value):
        n = ctypes.c_int64(count)
        return fn(kind, sigma, X.data_ptr(), Y.data_ptr(), W.data_ptr(), 0, go.data_ptr(), A, B, M, N, dim, buf.data_ptr(),
                  ctypes.c_void_p(partials) if partials else None, ctypes.byref(n), _lib._stream(X))
    assert call(kind=0) == 2
    assert call(dim=33) == 2
    assert call(partials=0) == 1
    assert call(count=need.value + 1) == 1 and call(count=need.value - 1) == 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote to its outputs"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(buf[:A * M * D + need.value]).all()) and bool(torch.isnan(buf[A * M * D + need.value:]).all())
    dX, dparam = _lib.HipBackend().static_adjoint_param(1, sigma, X, Y, W, go, gram)
    assert same_bits(dX.reshape(-1), buf[:A * M * D])[0]
    total = float(buf[A * M * D:A * M * D + need.value].sum()) / sigma ** 2
    assert abs(float(dparam) - total) <= 1e-14 * abs(total)
