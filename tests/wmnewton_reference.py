"""sa.sgdnet_wmnewton (SGDNET_MODE_WMNEWTON, sgdnet_amd/csrc/mnewton.hip: mnewton_wide_scale_kernel and
mnewton_wide_cd_kernel) restated in numpy, and the inputs its tests share: tests/test_gpu_wmnewton.py runs them on the
device, tests/test_wmnewton_host.py runs the restatement on the same inputs on the CPU.

The outer loop is tests/test_gpu_mnewton.py::numpy_mnewton_path's (state, the joint Hessian of all Q = K (p + 1)
coordinates, inner solve, accept / halve, the stopping rule).  The inner solve, about the iterate U_cur:
  start    U = U_cur, so g = H (U - U_cur) - q = -q exactly; the list is {c : c mod P < p, U_c != 0} and the K intercept
           coordinates c mod P == p when they are fitted (unpenalised, without threshold; frozen: never visited)
  screen   every penalised c outside the list gets the coordinate update from U_c = 0; those that would move join the
           list, which stays in ascending order of c
  sweep    mnewton mode's coordinate update over the list (a coordinate whose denominator is not positive stays; what
           the threshold leaves when |z| equals it but for rounding is an exact zero, for penalised coordinates with a
           positive denominator and not under ridge); a move by d does g += H[:, c] d for ALL coordinates, so g stays the
           full gradient.  The sweeps end as mnewton mode's do; then the screen runs again, and the solve is done when a
           screen adds nothing.
MAX_SWEEPS bounds the list sweeps of one solve; a solve cut short is continued by the next outer step."""
import numpy as np

import test_gpu_mnewton as tm

THRESH = tm.THRESH                        # what every GPU fit of the tests passes
LDS_BYTES = 160 * 1024
ALL_SETTINGS = tm.SETTINGS                # (intercept, standardize)
DEFAULTS = [(True, True)]
MIXES = tm.MIXES
MAX_HALVINGS, OBJECTIVE_SLACK, MAX_SWEEPS, NEGLIGIBLE = tm.MAX_HALVINGS, tm.OBJECTIVE_SLACK, tm.MAX_SWEEPS, tm.NEGLIGIBLE
TILE_COLS, TILE_ROWS = tm.TILE_COLS, tm.TILE_ROWS          # csrc/moments_device.hpp, read by tm.kernel_constants()
MAX_CLASSES = 99


def state_bytes(Q):
    """mnewton.hpp: g, U and diag H (3 Q doubles), Q list words, one bit per coordinate in whole words, the compaction's
    2 x 16 counts; Q = K (p + 1)"""
    return 24 * Q + 4 * Q + 4 * ((Q + 31) // 32) + 4 * 2 * 16


def derived_max_coordinates():
    """the largest Q that fits one workgroup's LDS"""
    Q = 1
    while state_bytes(Q + 1) <= LDS_BYTES:
        Q += 1
    return Q


MAX_COORDINATES = derived_max_coordinates()      # 5820


def max_features(K):
    """sgdnet_wmnewton_max_features(K): 5820 // K - 1 for 2 <= K <= 99, 0 otherwise"""
    return MAX_COORDINATES // K - 1 if 2 <= K <= MAX_CLASSES else 0


def tile_pairs(ncols):
    T = (ncols + 15) // 16
    return T * (T + 1) // 2


def row_chunks(n, p, K):
    """mnewton.hpp: wmnewton_row_chunks over ncols = p + 2 columns -- as many chunks as put about 1024 workgroups (tile
    pairs x class pairs a chunk) on the GPU, none shorter than 256 rows, one once a chunk alone has 1024"""
    wg = tile_pairs(p + 2) * (K * (K + 1) // 2)
    cap = 1 if wg >= 1024 else 1024 // wg
    return max(1, min((n + 255) // 256, cap))


def rows_per_chunk(n, p, K, tile_rows=None):
    """... and the rows of a chunk, rounded up to whole steps of tile_rows staged rows"""
    tile_rows = tile_rows or TILE_ROWS
    c = row_chunks(n, p, K)
    return ((n + c - 1) // c + tile_rows - 1) // tile_rows * tile_rows


def numpy_wide_mnewton_path(x, y, K, lam, mix, standardize=True, intercept=True, thresh=THRESH, maxit=1000):
    """(a0 (K, L), beta (K, p, L), dev_ratio (L), info); info: steps and codes per lambda, passes, halvings and list sweeps
    of the path, per lambda the most screens and list sweeps of one inner solve."""
    x = tm.dense(x)
    n, p = x.shape
    P, Q = p + 1, K * (p + 1)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    sd = np.where(var == 0, 1.0, np.sqrt(var)) if standardize else np.ones(p)
    m = mean if (standardize or intercept) else np.zeros(p)
    Z = np.column_stack([(x - m) / sd, np.ones(n)])
    yi = y.astype(int)
    Y = np.eye(K)[yi]
    b0 = tm.null_intercepts(y, K, intercept)
    u = np.zeros((K, P))
    u[:, p] = b0
    u = u.ravel()
    pen = np.tile(np.arange(P) < p, K)                            # penalised coordinates
    ridge = mix == 0

    def state(u):
        eta = Z @ u.reshape(K, P).T
        mx = eta.max(axis=1, keepdims=True)
        e = np.exp(eta - mx)
        s = e.sum(axis=1, keepdims=True)
        return e / s, (np.log(s[:, 0]) + mx[:, 0] - eta[np.arange(n), yi]).mean()

    def penalty(u, l1, l2):
        return l2 * 0.5 * (u[pen] ** 2).sum() + l1 * np.abs(u[pen]).sum()

    pr0 = np.bincount(yi, minlength=K) / n if intercept else np.full(K, 1.0 / K)
    nulldev = -2.0 * np.log(pr0[yi]).sum()
    mu, loss = state(u)
    info = dict(halvings=0, steps=[], codes=[], passes=1, total_sweeps=0, screens=[], sweeps=[])
    a0, beta, dev = [], [], []
    for l in lam:
        l1, l2 = (0.0 if ridge else mix * l), (1 - mix) * l
        objective = loss + penalty(u, l1, l2)
        steps, converged, most_screens, most_sweeps = 0, False, 0, 0
        while steps < maxit and not converged:
            H = np.empty((Q, Q))
            for k in range(K):
                for kk in range(k, K):
                    wgt = mu[:, k] * ((1.0 if k == kk else 0.0) - mu[:, kk])
                    blk = (Z * wgt[:, None]).T @ Z / n
                    H[k * P:(k + 1) * P, kk * P:(kk + 1) * P] = blk
                    H[kk * P:(kk + 1) * P, k * P:(k + 1) * P] = blk
            q = (Z.T @ (Y - mu) / n).T.ravel()
            c, g = u.copy(), -q
            diag = np.diag(H).copy()
            in_list = np.where(pen, c != 0.0, bool(intercept))
            inner = negligible = False
            sweeps = screens = 0
            while True:
                # the screen: the coordinate update from U_c = 0 for every penalised coordinate at once
                z, den = -g, diag + l2
                nu0 = z if ridge else np.where(z > l1, z - l1, np.where(z < -l1, z + l1, 0.0))
                with np.errstate(divide="ignore", invalid="ignore"):
                    nu0 = np.where(den > 0, nu0 / den, 0.0)                        # (a coordinate that stays, stays at 0)
                if not ridge:
                    nu0 = np.where((den > 0) & (nu0 * nu0 * diag <= NEGLIGIBLE ** 2), 0.0, nu0)
                added = pen & (nu0 != 0.0) & ~in_list
                screens += 1
                if screens > 1 and not added.any():
                    inner = True
                    break
                in_list |= added
                live = np.flatnonzero(in_list)
                met = False
                while sweeps < MAX_SWEEPS and not met:
                    change = size = eta_sq = 0.0
                    for j in live:
                        hjj, cj = diag[j], c[j]
                        z, den = hjj * cj - g[j], hjj + (l2 if pen[j] else 0.0)
                        nu = z
                        if pen[j] and not ridge:
                            nu = z - l1 if z > l1 else (z + l1 if z < -l1 else 0.0)
                        nu = nu / den if den > 0 else cj
                        if pen[j] and not ridge and den > 0 and nu * nu * hjj <= NEGLIGIBLE ** 2:
                            nu = 0.0                                                # the threshold's rounding residue: exactly 0
                        d = nu - cj
                        change, size, eta_sq = max(change, abs(d)), max(size, abs(nu)), max(eta_sq, nu * nu * hjj)
                        if d != 0.0:
                            c[j] = nu
                            g += H[j] * d                                           # (H is symmetric: row j is column j)
                    sweeps += 1
                    negligible = eta_sq <= NEGLIGIBLE ** 2                          # zero to rounding (newton.hpp)
                    met = (size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible
                if not met:
                    break
            most_screens, most_sweeps = max(most_screens, screens), max(most_sweeps, sweeps)
            info["total_sweeps"] += sweeps
            mu, cl = state(c)
            info["passes"] += 1
            candidate = cl + penalty(c, l1, l2)
            h = 0
            while h < MAX_HALVINGS and np.abs(c - u).max() > 0 and not candidate <= objective + OBJECTIVE_SLACK * abs(objective):
                c = u + 0.5 * (c - u)
                mu, cl = state(c)
                info["passes"] += 1
                candidate = cl + penalty(c, l1, l2)
                h += 1
                negligible = False
            info["halvings"] += h
            change, size = np.abs(c - u).max(), np.abs(c).max()
            u, loss, objective = c, cl, candidate
            steps += 1
            converged = inner and ((size == 0 and change == 0) or (size != 0 and change / size <= thresh) or negligible)
        info["steps"].append(steps)
        info["codes"].append(0 if converged else 1)
        info["screens"].append(most_screens)
        info["sweeps"].append(most_sweeps)
        U = u.reshape(K, P)
        b = U[:, :p] / sd
        icpt = U[:, p] - b @ m if intercept else b0.copy()
        a0.append(icpt - icpt.mean() if intercept else icpt)
        beta.append(b)
        dev.append(1.0 - 2.0 * n * loss / nulldev)
    return np.array(a0).T, np.moveaxis(np.array(beta), 0, 2), np.array(dev), info


automatic_lambdas = tm.automatic_lambdas
problem = tm.problem


# ---- the inputs: (n, p, K); p = None: the feature limit of K ----
BEYOND_MNEWTON = [(120, 99, 2), (90, 66, 3)]                     # Q = 200, 201: the first Q mode = mnewton refuses
ODD_Q = [(90, 84, 3)]                                            # Q = 255: the last slot of wide_column_move holds one entry
STRIDE_256 = [(90, 127, 2), (90, 128, 2)]                        # Q = 256, 258: one stride of the 256-lane compaction, and past it
STRIDE_1024 = [(65, 340, 3), (65, 511, 2), (65, 512, 2)]         # Q = 1023, 1024, 1026: the width rule and the 1024-lane stride
MANY_CLASSES = [(150, 30, 10), (300, 2, 99)]                     # Q = 310, 297
TILE_SHAPES = [(90, TILE_COLS - 3, 3), (90, TILE_COLS - 2, 3), (90, TILE_COLS - 1, 3)]       # p + 2 = 15, 16, 17 at one tile edge
ROW_SHAPES = [(n, 3, 3) for n in (TILE_ROWS - 1, TILE_ROWS + 1, 255, 256, 257)]             # the staging step; the second row chunk
# Q = 5820, 5820, 5742.  (99 classes take 200 rows, not 40: problem() gives every class two members -- a class without a
# member has no null-model intercept, and sgdnet()'s validation refuses a class of one -- so 198 rows are the fewest.)
LIMIT_SHAPES = [(40, None, 2), (40, None, 3), (200, None, 99)]
SMALL_SHAPES = BEYOND_MNEWTON + ODD_Q + STRIDE_256 + STRIDE_1024 + MANY_CLASSES + TILE_SHAPES + ROW_SHAPES
SHAPES = SMALL_SHAPES + LIMIT_SHAPES
# where mode = mnewton runs too
BOTH_MODES = [(120, 5, 2), (160, 5, 4), (200, 6, 5), (300, 65, 3)] + TILE_SHAPES
# beyond mnewton's limit the curvature guard compares with the restatement's own pass count
PASS_GUARD_SHAPES = [(90, 66, 3), (150, 30, 10), (90, 127, 2)]
LIMIT_KS = [-3, 0, 1, 2, 3, 4, 5, 10, 20, 50, 99, 100, 2147483647]
LIMIT_TABLE = {2: 2909, 3: 1939, 4: 1454, 5: 1163, 10: 581, 20: 290, 50: 115, 99: 57}


def features_of(shape):
    return shape[1] if shape[1] is not None else max_features(shape[2])


def path_of(shape, mix):
    """(nlambda, lambda_min_ratio) of the automatic path a shape is fitted with.  With more coordinates per class than
    samples the classes separate: the unpenalised end of the path does not exist, and the ratio keeps away from it."""
    n, p, K = shape
    if p is None:
        return (2, 0.3) if mix == 0.0 else (3, 0.2)      # (ridge: every sweep moves all coordinates)
    if mix == 0.0 and K * (p + 1) >= 1000:
        return (3, 0.1)                                  # (ridge: every sweep moves all 1023 .. 1026 coordinates, in four settings)
    if p >= n // 2 or K >= 10:
        return (4, 1e-2) if mix == 0.0 else (4, 0.1)
    return (5, 1e-2)


def settings_of(shape):
    return ALL_SETTINGS if shape[1] is not None else DEFAULTS
