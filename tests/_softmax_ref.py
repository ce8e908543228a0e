"""Float64 ground truth of the linear probe (no test in here): the multinomial logistic-regression objective sklearn's
LogisticRegression(C=1, penalty="l2", fit_intercept=True) minimises, its gradient, a tight optimiser, the variance
formulas of the reference's compute_intra_inter_variance, and the two seeded problems of tests/golden/
linear_probe_ref.npz (inputs are regenerated from the seed; the fixture holds their sha256)."""
import hashlib

import numpy as np

# name -> (seed, n_train, n_test, d, classes, noise per coordinate)
PROBLEMS = {
    "p10": (20240, 4000, 2000, 256, 10, 5.5),
    "p27": (20241, 6000, 2000, 768, 27, 9.5),
}


def make_problem(name):
    """Clustered unit-norm fp32 rows: (x_train, y_train, x_test, y_test)."""
    seed, ntr, nte, d, c, noise = PROBLEMS[name]
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((c, d))
    y = rng.integers(0, c, ntr + nte)
    x = centers[y] + noise * rng.standard_normal((ntr + nte, d))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    y = y.astype(np.int64)
    return x[:ntr].copy(), y[:ntr].copy(), x[ntr:].copy(), y[ntr:].copy()


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def data_term(w, b, x, y):
    """(sum_i logsumexp(z_i) - z_i,y_i,  d/dW,  d/db) in float64, z = x w^T + b."""
    x = np.asarray(x, dtype=np.float64)
    z = x @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(axis=1, keepdims=True)
    lse = (m + np.log(s))[:, 0]
    rows = np.arange(x.shape[0])
    f = float(np.sum(lse - z[rows, y]))
    p = e / s
    p[rows, y] -= 1.0
    return f, p.T @ x, p.sum(axis=0)


def objective(w, b, x, y):
    """F = data term + 0.5 ||W||^2 and its gradient."""
    f, gw, gb = data_term(w, b, x, y)
    w = np.asarray(w, dtype=np.float64)
    return f + 0.5 * float(np.sum(w * w)), gw + w, gb


def optimum(x, y, c):
    """The float64 minimiser (W [c, d], b [c], F): scipy L-BFGS-B, gtol=1e-10, ftol=1e-16."""
    from scipy.optimize import minimize
    d = x.shape[1]
    x64 = np.asarray(x, dtype=np.float64)

    def fun(t):
        f, gw, gb = objective(t[: c * d].reshape(c, d), t[c * d:], x64, y)
        return f, np.concatenate([gw.ravel(), gb])

    r = minimize(fun, np.zeros(c * d + c), jac=True, method="L-BFGS-B",
                 options={"gtol": 1e-10, "ftol": 1e-16, "maxiter": 100000, "maxfun": 200000, "maxcor": 30})
    return r.x[: c * d].reshape(c, d), r.x[c * d:], float(r.fun)


def centred_logits(w, b, x):
    z = np.asarray(x, dtype=np.float64) @ np.asarray(w, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    return z - z.mean(axis=1, keepdims=True)


def variance(features, labels, dtype=np.float64):
    """The reference's loop (HairPretraining/src/classification_engine.py:241-262) at the given precision."""
    features = np.asarray(features, dtype=dtype)
    classes = np.unique(labels)
    g = np.mean(features, axis=0)
    intra = inter = 0.0
    for c in classes:
        f = features[labels == c]
        m = np.mean(f, axis=0)
        intra += np.mean(np.sum((f - m) ** 2, axis=1))
        inter += np.sum((m - g) ** 2)
    intra /= len(classes)
    inter /= len(classes)
    return float(intra), float(inter), float(inter / (intra + 1e-8))
