"""Writes tests/golden/linear_probe_ref.npz: for the two seeded problems of tests/_softmax_ref.py, a sha256 of the
generated inputs, the float64 optimum (W, b, F), scikit-learn's coef_ / intercept_ / n_iter_ / test predictions for the
reference's LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial"), and the three variance
values of train + test in float64.  Run from the repository root:  python tests/golden/make_linear_probe_ref.py"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _softmax_ref as ref  # noqa: E402


def main():
    import sklearn
    from sklearn.linear_model import LogisticRegression
    out = {"sklearn_version": np.array(sklearn.__version__)}
    for name in ref.PROBLEMS:
        xtr, ytr, xte, yte = ref.make_problem(name)
        c = ref.PROBLEMS[name][4]
        w, b, f = ref.optimum(xtr, ytr, c)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            clf = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit(xtr, ytr)
        intra, inter, ratio = ref.variance(np.concatenate([xtr, xte]), np.concatenate([ytr, yte]))
        out.update({
            f"{name}_sha256": np.array(ref.digest(xtr, ytr, xte, yte)),
            f"{name}_w_opt": w, f"{name}_b_opt": b, f"{name}_f_opt": np.float64(f),
            f"{name}_sk_coef": clf.coef_.astype(np.float64), f"{name}_sk_intercept": clf.intercept_.astype(np.float64),
            f"{name}_sk_n_iter": np.int64(clf.n_iter_[0]), f"{name}_sk_pred": clf.predict(xte).astype(np.int64),
            f"{name}_variance": np.array([intra, inter, ratio], dtype=np.float64),
        })
        g = ref.objective(w, b, xtr, ytr)
        print(name, "F_opt", f, "max|grad|", max(np.abs(g[1]).max(), np.abs(g[2]).max()), "sk n_iter", clf.n_iter_[0],
              "sk acc", float((clf.predict(xte) == yte).mean()))
    np.savez_compressed(os.path.join(HERE, "linear_probe_ref.npz"), **out)


if __name__ == "__main__":
    main()
