"""Plain numpy f64 reference for the grouped multinomial penalty of sa.sgdnet_mnewton / sa.sgdnet_wmnewton, in the
standardised coordinates the driver penalises in (sgdnet_amd/kkt.py), z_j = (x_j - mean_j) / sd_j:
    F(W, b) = mean_i [log sum_k e^eta_ik - eta_{i, y_i}] + lambda ((1 - mix) / 2 |W|^2 + mix sum_j |w_.j|_2),  eta = b + z W,
W (p, K), b (K) unpenalised (held at 0 without an intercept).  Nothing here knows the library."""
import numpy as np

# (n, p, K): one block; a few; an even K; several strides of 64 lanes; Q = 198, the narrow limit at K = 3, on 256 lanes.
# WIDE_ONLY: Q = 213, beyond the narrow limit; K = 5 with an odd Q.
SHAPES = [(60, 1, 2), (120, 5, 3), (160, 5, 4), (200, 33, 3), (300, 65, 3)]
WIDE_ONLY = [(300, 70, 3), (200, 40, 5)]
MIXES = [1.0, 0.5]
N_LAMBDA, MIN_RATIO, THRESH = 8, 0.02, 1e-10
FLOOR = 1e-13      # solve() stops at this KKT residual: rounding in the gradient is a few 1e-17 a row, over up to 300 rows


def problem(n, p, K):
    """x (n, p) with unequal column scales and some correlation, y (n) class codes from a softmax model on a few features"""
    rng = np.random.default_rng(1000 * n + 10 * p + K)
    x = rng.normal(size=(n, p)) + 0.4 * rng.normal(size=(n, 1))
    x = x * rng.uniform(0.5, 2.0, size=p) + rng.normal(size=p)
    w = np.zeros((p, K))
    live = rng.choice(p, size=min(p, 4), replace=False)
    w[live] = rng.normal(size=(live.size, K))
    eta = standardised(x)[0] @ w
    pr = np.exp(eta - eta.max(1, keepdims=True))
    pr /= pr.sum(1, keepdims=True)
    y = np.array([rng.choice(K, p=row) for row in pr])
    y[:2 * K] = np.repeat(np.arange(K), 2)                     # every class at least twice
    return x, y.astype(np.float64)


def standardised(x):
    return (x - x.mean(0)) / x.std(0), x.mean(0), x.std(0)


def objective(z, y, W, b, lam, mix):
    eta = z @ W + b
    mx = eta.max(1)
    loss = np.mean(np.log(np.exp(eta - mx[:, None]).sum(1)) + mx - eta[np.arange(len(y)), y.astype(int)])
    return loss + lam * ((1.0 - mix) / 2.0 * (W ** 2).sum() + mix * np.sqrt((W ** 2).sum(1)).sum())


def gradient(z, y, W, b):
    """(dF/dW (p, K), dF/db (K)) of the loss"""
    eta = z @ W + b
    r = np.exp(eta - eta.max(1, keepdims=True))
    r /= r.sum(1, keepdims=True)
    r[np.arange(len(y)), y.astype(int)] -= 1.0
    return z.T @ r / len(y), r.mean(0)


def kkt_residual(z, y, W, b, lam, mix, intercept=True):
    """the largest violation of the group optimality conditions over the features, and of the intercepts' stationarity"""
    g, g0 = gradient(z, y, W, b)
    l1, l2 = mix * lam, (1.0 - mix) * lam
    nrm = np.sqrt((W ** 2).sum(1))
    unit = np.divide(W, nrm[:, None], out=np.zeros_like(W), where=nrm[:, None] > 0)
    on = np.sqrt(((g + l2 * W + l1 * unit) ** 2).sum(1))
    off = np.maximum(np.sqrt((g ** 2).sum(1)) - l1, 0.0)
    return max(np.where(nrm > 0, on, off).max(), np.abs(g0).max() if intercept else 0.0)


def user_lambdas(z, y, K, mix, intercept=True):
    """N_LAMBDA lambdas from the smallest at which W = 0 is optimal, max_j |g_.j|_2 / mix at the null model, down"""
    g, _ = gradient(z, y, np.zeros((z.shape[1], K)), np.log(np.bincount(y.astype(int), minlength=K) / len(y)) * intercept)
    return np.sqrt((g ** 2).sum(1)).max() / mix * np.logspace(0.0, np.log10(MIN_RATIO), N_LAMBDA)


def solve(z, y, K, lambdas, mix, intercept=True, max_iter=200000):
    """[(W, b, residual)] per lambda: accelerated proximal gradient, warm started along the path, run until the residual is
    below FLOOR.  Step 1 / L, L = max(lambda_max(z'z / n), 1) / 2 + l2 (the softmax Hessian is at most I / 2); the momentum
    restarts when the objective rises."""
    L0 = 0.5 * max(np.linalg.eigvalsh(z.T @ z / len(y)).max(), 1.0)
    W, b, out = np.zeros((z.shape[1], K)), np.log(np.bincount(y.astype(int), minlength=K) / len(y)) * intercept, []
    for lam in lambdas:
        l1, l2 = mix * lam, (1.0 - mix) * lam
        step = 1.0 / (L0 + l2)
        Wy, by, t, f_old = W.copy(), b.copy(), 1.0, objective(z, y, W, b, lam, mix)
        for it in range(max_iter):
            g, g0 = gradient(z, y, Wy, by)
            V = Wy - step * (g + l2 * Wy)
            Wn = V * np.maximum(0.0, 1.0 - step * l1 / np.maximum(np.sqrt((V ** 2).sum(1, keepdims=True)), 1e-300))
            bn = by - step * g0 if intercept else by
            f_new = objective(z, y, Wn, bn, lam, mix)
            if f_new > f_old:                                  # restart from the last accepted point
                Wy, by, t, f_old = W.copy(), b.copy(), 1.0, np.inf
                continue
            tn = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
            Wy, by = Wn + (t - 1.0) / tn * (Wn - W), bn + (t - 1.0) / tn * (bn - b)
            W, b, t, f_old = Wn, bn, tn, f_new
            if it % 20 == 0 and kkt_residual(z, y, W, b, lam, mix, intercept) <= FLOOR:
                break
        out.append((W.copy(), b.copy(), kkt_residual(z, y, W, b, lam, mix, intercept)))
    return out
