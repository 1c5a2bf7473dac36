"""Generate tests/golden/truncated_levels.npz by running the REAL reference's truncated_sig_kernel (sigkernel/transformers.py:201-236)
once per level, with the unit vectors as ``sigma``: the reference has no per-level output, but its kernel is linear in the weights, so
``K(sigma = e_m)`` is level m's term.

Container-only, like make_golden_truncated.py: needs the reference checkout (oracle/build_ref.py: REF) with scipy and sklearn.  The
reference's transformers.py is loaded BY FILE PATH -- importing its package pulls in numba -- and nothing of its text is kept: the file
written holds the inputs, the arguments and the reference's outputs, data only.

The cases are tiny (the reference takes minutes beyond a dozen steps): a few pairs of <= 12 steps; fp64 and fp32, num_levels 1..6, order
in {-1, 1, 2, 3}, len_x != len_y, dim 1 / 3 / 8, A != B and -- for the paired checks -- A == B.  Steps are scaled to norm ~0.2-0.5 so that
no level vanishes or dominates."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.build_ref import REF  # noqa: E402

spec = importlib.util.spec_from_file_location("reference_transformers", os.path.join(REF, "sigkernel", "transformers.py"))
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

# (A, B, len_x, len_y, dim, num_levels, order, dtype)
CASES = [
    (3, 2, 7, 5, 3, 1, -1, "f64"),
    (2, 3, 6, 9, 1, 2, -1, "f64"),
    (3, 3, 8, 5, 8, 4, -1, "f64"),
    (2, 2, 5, 12, 3, 5, -1, "f64"),
    (2, 2, 6, 4, 3, 6, -1, "f64"),
    (3, 2, 9, 6, 3, 4, 1, "f64"),
    (2, 3, 7, 10, 8, 6, 1, "f64"),
    (3, 3, 8, 6, 1, 4, 2, "f64"),
    (2, 3, 6, 7, 8, 5, 2, "f64"),
    (2, 2, 7, 5, 3, 5, 3, "f64"),
    (3, 2, 5, 8, 8, 6, 3, "f64"),
    (3, 2, 7, 5, 3, 3, -1, "f32"),
    (2, 3, 6, 9, 8, 5, 2, "f32"),
    (2, 2, 10, 4, 1, 4, 1, "f32"),
    (3, 2, 5, 7, 3, 6, 3, "f32"),
]


def main():
    rng = np.random.default_rng(20261018)
    out = {"n_cases": np.int64(len(CASES))}
    for c, (A, B, M, N, D, L, order, dt) in enumerate(CASES):
        dtype = np.float64 if dt == "f64" else np.float32

        def steps(n, m):
            v = rng.standard_normal((n, m, D))
            v *= rng.uniform(0.2, 0.5, (n, m, 1)) / np.linalg.norm(v, axis=2, keepdims=True)
            return v.astype(dtype)

        X, Y = steps(A, M), steps(B, N)
        levels = []
        for m in range(L + 1):
            e = np.zeros(L + 1, dtype=dtype)
            e[m] = 1
            K = np.asarray(ref.truncated_sig_kernel(X.copy(), Y.copy(), L, sigma=e, order=order))
            assert K.shape == (A, B) and np.isfinite(K).all()
            levels.append(K)
        levels = np.stack(levels, 0)
        assert np.array_equal(levels[0], np.ones((A, B), dtype=levels.dtype))
        k = "c%02d_" % c
        out[k + "X"], out[k + "Y"], out[k + "levels"] = X, Y, levels
        out[k + "num_levels"], out[k + "order"] = np.int64(L), np.int64(order)
        print(c, (A, B, M, N, D, L, order, dt), [float(np.abs(v).max()) for v in levels], levels.dtype)
    np.savez_compressed(os.path.join(HERE, "truncated_levels.npz"), **out)


if __name__ == "__main__":
    main()
