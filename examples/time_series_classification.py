#!/usr/bin/env python3
"""Time-series classification with a precomputed signature-kernel Gram matrix -- the pipeline of the reference's
examples/time_series_classification.py:94 and :189-202 (transform -> compute_Gram(sym=True) -> sklearn SVC with
kernel='precomputed', hyper-parameters by cross-validated grid search), on synthetic two-class paths: the UCR/UEA data
sets the reference downloads through tslearn are not available offline.

    python examples/time_series_classification.py [--n-train 120] [--n-test 80] [--length 60] [--ragged]
    python examples/time_series_classification.py --truncated [--normalize | --robust] [--static rbf [--rbf-sigma S]]

--ragged: the variable-length variant -- every series is cut at a random length in [length / 2, length], the batch is padded by
pad_paths and the Gram matrices come from compute_Gram_ragged.

--truncated: the truncated signature kernel of the transformed series' steps (truncated_sig_kernel, four levels) in place of the PDE
kernel; --normalize divides it by sqrt(k(x, x) k(y, y)) (normalize=True: the A + B self-kernels come from one paired launch each).
--robust: Chevyrev and Oberhauser's robust normalisation instead -- truncated_sig_kernel_levels (the level terms of one sweep) ->
truncated_robust_scales (a scale per path from its paired self levels) -> truncated_from_levels (the kernel of the rescaled paths).
--static rbf: the truncated kernel lifted through an RBF static kernel on the series' POINTS, as Kiraly and Oberhauser state it --
TruncatedSigKernel(4, static_kernel=RBFKernel(S)).compute_Gram on the transformed series themselves, one HIP sweep per matrix;
--normalize divides by the self-kernels from compute_kernel.  (The robust normalisation rescales steps and has no lifted form.)

Class 0: Brownian paths with a slow sinusoidal drift; class 1: the same noise with the drift's frequency doubled.
Runs on an MI355X (the Gram matrices come from the HIP kernels; there is no CPU fallback).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sigkernel_amd as sigkernel  # noqa: E402


def make_dataset(n, length, seed, noise=0.35):
    """(n, length, 1) float64 paths and (n,) integer labels, two balanced classes."""
    rng = np.random.default_rng(seed)
    y = np.arange(n) % 2
    t = np.linspace(0.0, 1.0, length)
    phase = rng.uniform(0, 2 * np.pi, size=(n, 1))
    drift = np.sin(2 * np.pi * (1 + y)[:, None] * t[None, :] + phase)
    walk = np.cumsum(rng.normal(scale=noise / np.sqrt(length), size=(n, length)), axis=1)
    x = (drift + walk)[:, :, None]
    return x, y


def fit_signature_svc(x_train, y_train, device, sigmas=(0.25, 0.5, 1.0), at=True, ll=False, scale=0.1, dyadic_order=0,
                      cv=5, dtype=torch.float64, lens=None):
    """Grid search over the RBF sigma of the static kernel and the SVC's C, as the reference does
    (examples/time_series_classification.py:150-202).  Returns (best cv score, sigma, fitted GridSearchCV, train tensor)."""
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC
    if lens is not None and ll:
        raise ValueError("lens count the points of the untransformed series: the lead-lag transform changes the length")
    x_train = x_train / np.abs(x_train).max()                                    # :88
    xt = sigkernel.transform(torch.tensor(x_train, dtype=dtype, device=device), at=at, ll=ll, scale=scale)   # :94
    best = (-1.0, None, None)
    for sigma in sigmas:
        signature_kernel = sigkernel.SigKernel(sigkernel.RBFKernel(sigma=sigma), dyadic_order=dyadic_order)     # :186-189
        if lens is None:
            G_train = signature_kernel.compute_Gram(xt, xt, sym=True).cpu().numpy()                            # :192
        else:       # series of unequal length, padded at their ends
            G_train = signature_kernel.compute_Gram_ragged(xt, xt, lens, lens, sym=True).cpu().numpy()
        svc = SVC(kernel="precomputed", decision_function_shape="ovo")                                         # :195
        model = GridSearchCV(estimator=svc, param_grid={"C": np.logspace(0, 4, 5)}, cv=cv, n_jobs=1)           # :196
        model.fit(G_train, y_train)                                                                            # :197
        if model.best_score_ > best[0]:
            best = (float(model.best_score_), sigma, model)
    return best + (xt,)


def predict(model, sigma, xt_train, x_test, x_train_max, device, at=True, ll=False, scale=0.1, dyadic_order=0,
            dtype=torch.float64, lens_test=None, lens_train=None):
    """Test-vs-train Gram matrix and the SVC's predictions (examples/time_series_classification.py:262-281)."""
    if lens_test is not None and ll:
        raise ValueError("lens count the points of the untransformed series: the lead-lag transform changes the length")
    xs = sigkernel.transform(torch.tensor(x_test / x_train_max, dtype=dtype, device=device), at=at, ll=ll, scale=scale)
    signature_kernel = sigkernel.SigKernel(sigkernel.RBFKernel(sigma=sigma), dyadic_order=dyadic_order)
    if lens_test is None:
        G_test = signature_kernel.compute_Gram(xs, xt_train, sym=False).cpu().numpy()
    else:
        G_test = signature_kernel.compute_Gram_ragged(xs, xt_train, lens_test, lens_train).cpu().numpy()
    return model.predict(G_test)


def robust_gram(X, Y, num_levels):
    """The robustly normalised truncated kernel matrix of two step batches: levels -> scales -> truncated_from_levels, three sweeps."""
    lam_x = sigkernel.truncated_robust_scales(sigkernel.truncated_sig_kernel_levels(X, X, num_levels, paired=True))
    lam_y = lam_x if Y is X else sigkernel.truncated_robust_scales(sigkernel.truncated_sig_kernel_levels(Y, Y, num_levels, paired=True))
    return sigkernel.truncated_from_levels(sigkernel.truncated_sig_kernel_levels(X, Y, num_levels), 1., lam_x, lam_y)


def lifted_gram(tk, X, Y, normalize):
    """The Gram matrix of a TruncatedSigKernel with a static kernel on two batches of PATHS, divided by sqrt(k(x, x) k(y, y)) on request."""
    K = tk.compute_Gram(X, Y)
    if normalize:
        kx = tk.compute_kernel(X, X)
        ky = kx if Y is X else tk.compute_kernel(Y, Y)
        K = K / torch.sqrt(kx[:, None] * ky[None, :])
    return K


def truncated_svc(x_train, y_train, x_test, device, normalize, num_levels=4, cv=5, robust=False, static=None, rbf_sigma=1.0):
    """The same pipeline with truncated_sig_kernel on the STEPS of the time-augmented series -- static="rbf": with the RBF-lifted
    TruncatedSigKernel on their POINTS: (cv score, C, test predictions)."""
    from sklearn.model_selection import GridSearchCV
    from sklearn.svm import SVC
    top = np.abs(x_train).max()
    paths = [sigkernel.transform(torch.tensor(x / top, dtype=torch.float64, device=device), at=True, ll=False, scale=1.0) for x in (x_train, x_test)]
    steps = [torch.diff(x, dim=1) for x in paths]
    if static == "rbf":
        tk = sigkernel.TruncatedSigKernel(num_levels, static_kernel=sigkernel.RBFKernel(rbf_sigma))
        G_train = lifted_gram(tk, paths[0], paths[0], normalize).cpu().numpy()
        G_test = lifted_gram(tk, paths[1], paths[0], normalize).cpu().numpy()
    elif robust:
        G_train, G_test = robust_gram(steps[0], steps[0], num_levels).cpu().numpy(), robust_gram(steps[1], steps[0], num_levels).cpu().numpy()
    else:
        G_train = sigkernel.truncated_sig_kernel(steps[0], steps[0], num_levels, normalize=normalize).cpu().numpy()
        G_test = sigkernel.truncated_sig_kernel(steps[1], steps[0], num_levels, normalize=normalize).cpu().numpy()
    model = GridSearchCV(estimator=SVC(kernel="precomputed", decision_function_shape="ovo"), param_grid={"C": np.logspace(0, 4, 5)}, cv=cv, n_jobs=1)
    model.fit(G_train, y_train)
    return float(model.best_score_), model.best_params_["C"], model.predict(G_test)


def cut_and_pad(x, seed):
    """Cut every series of x (n, length, channels) at a random length in [length / 2, length] and pad the batch back to `length`
    (pad_paths repeats the last point; the padding never reaches a result).  Returns the padded array and the lengths."""
    if x.ndim != 3:
        raise ValueError("x must have shape (n, length, channels)")
    rng = np.random.default_rng(seed)
    lens = rng.integers(x.shape[1] // 2, x.shape[1] + 1, size=x.shape[0])
    padded, lens_t = sigkernel.pad_paths([torch.tensor(x[i, :n]) for i, n in enumerate(lens)])
    # train and test keep ONE padded length (the original): transform(at=True) adds time as linspace(0, 1, padded length), so its step
    # -- part of every path's increments -- must be the same in both sets
    tail = padded[:, -1:].expand(-1, x.shape[1] - padded.shape[1], -1)
    return torch.cat((padded, tail), dim=1).numpy(), lens_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-train", type=int, default=120)
    ap.add_argument("--n-test", type=int, default=80)
    ap.add_argument("--length", type=int, default=60)
    ap.add_argument("--ragged", action="store_true", help="series of unequal length: pad_paths -> compute_Gram_ragged(sym=True) -> SVC")
    ap.add_argument("--truncated", action="store_true", help="truncated_sig_kernel of the series' steps instead of the PDE kernel")
    ap.add_argument("--normalize", action="store_true", help="with --truncated: k(x, y) / sqrt(k(x, x) k(y, y))")
    ap.add_argument("--robust", action="store_true", help="with --truncated: the robust normalisation, from the level terms of one sweep")
    ap.add_argument("--static", choices=["rbf"], default=None, help="with --truncated: lift the kernel through this static kernel on the points")
    ap.add_argument("--rbf-sigma", type=float, default=1.0, help="with --static rbf: the RBF kernel's sigma")
    args = ap.parse_args()
    if args.static and (not args.truncated or args.robust):
        raise SystemExit("--static goes with --truncated, plain or with --normalize")
    if (args.normalize or args.robust) and not args.truncated or args.truncated and args.ragged or args.normalize and args.robust:
        raise SystemExit("--normalize or --robust (one of them) goes with --truncated, and --truncated takes series of one length")
    if not torch.cuda.is_available():
        raise SystemExit("this example needs an MI355X (sigkernel_amd has no CPU path)")
    device = torch.device("cuda", 0)
    x_train, y_train = make_dataset(args.n_train, args.length, seed=0)
    x_test, y_test = make_dataset(args.n_test, args.length, seed=1)
    if args.truncated:
        score, C, pred = truncated_svc(x_train, y_train, x_test, device, args.normalize, robust=args.robust, static=args.static,
                                       rbf_sigma=args.rbf_sigma)
        acc = float(np.mean(pred == y_test))
        how = " (normalised)" if args.normalize else " (robustly normalised)" if args.robust else ""
        how = (", RBF(%g) lift" % args.rbf_sigma if args.static else "") + how
        print("truncated signature kernel%s + SVC: cv accuracy %.3f (C %g), test accuracy %.3f" % (how, score, C, acc))
        return acc
    if args.ragged:
        # (the transform -- time as a channel -- acts point by point, so it commutes with the padding)
        x_train, len_train = cut_and_pad(x_train, seed=2)
        x_test, len_test = cut_and_pad(x_test, seed=3)
        score, sigma, model, xt = fit_signature_svc(x_train, y_train, device, lens=len_train)
        pred = predict(model, sigma, xt, x_test, np.abs(x_train).max(), device, lens_test=len_test, lens_train=len_train)
    else:
        score, sigma, model, xt = fit_signature_svc(x_train, y_train, device)
        pred = predict(model, sigma, xt, x_test, np.abs(x_train).max(), device)
    acc = float(np.mean(pred == y_test))
    print("signature PDE kernel + SVC: cv accuracy %.3f (sigma %.2f, C %g), test accuracy %.3f"
          % (score, sigma, model.best_params_["C"], acc))
    return acc


if __name__ == "__main__":
    main()
