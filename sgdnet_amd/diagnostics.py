"""Diagnostics (include/sgdnet_hip.h "Diagnostics"): what a fit's once-per-fit device setup passes
(sgdnet_amd/csrc/setup_device.hip) and the passes of one outer step of Newton mode (sgdnet_amd/csrc/newton.hip) and of
multinomial Newton mode (sgdnet_amd/csrc/mnewton.hip), narrow and wide, and the stages of the covariance family
(sgdnet_amd/csrc/covariance.hip), one fit or a cross-validation, leave on the device, copied back pass by pass.
Used by the tests; a fit never calls these."""
import ctypes as C
from types import SimpleNamespace

import numpy as np

from . import _lib
from ._lib import check, dptr

OVF_STRIDE = 256      # bytes of one overflow record (batched_device.hpp)
MAX_REC_STRIDE = 6400  # a cap of 512 entries at rec_align <= 256


def setup_probe_sparse(x, ymap, y, standardize=True, rec_align=128, device=0):
    """x: scipy.sparse matrix, n x p (converted to CSC as sgdnet() does); ymap: (n, cols); y: (y_rows, n) as the solvers
    read it.  Returns center, scale, max_mean_sq, xty (p, cols), sptr, sidx, sval, max_sqnorm, rec_stride, rec_cap,
    rec_val_off, n_ovf, rec (uint8, n * rec_stride), ovf (uint8, 256 * n_ovf), l_f."""
    x = x.tocsc()
    n, p = x.shape
    colptr = np.ascontiguousarray(x.indptr, dtype=np.int32)
    rowidx = np.ascontiguousarray(x.indices, dtype=np.int32)
    vals = np.ascontiguousarray(x.data, dtype=np.float64)
    nnz = int(colptr[-1])
    ymap = np.asfortranarray(np.asarray(ymap, dtype=np.float64).reshape(n, -1))
    y = np.asfortranarray(np.asarray(y, dtype=np.float64).reshape(-1, n))
    cols, y_rows = ymap.shape[1], y.shape[0]
    csc = _lib.Csc()
    csc.n_rows, csc.n_cols = n, p
    csc.colptr = colptr.ctypes.data_as(C.POINTER(C.c_int32))
    csc.rowidx = rowidx.ctypes.data_as(C.POINTER(C.c_int32))
    csc.values = dptr(vals)
    o = SimpleNamespace(center=np.empty(p), scale=np.empty(p), xty=np.empty((p, cols), order="F"),
                        sptr=np.empty(n + 1, dtype=np.int64), sidx=np.empty(max(nnz, 1), dtype=np.int32),
                        sval=np.empty(max(nnz, 1)), rec=np.empty(n * MAX_REC_STRIDE, dtype=np.uint8),
                        ovf=np.empty((nnz // 20 + n) * OVF_STRIDE, dtype=np.uint8))
    pr = _lib.SetupProbe()
    pr.center, pr.scale, pr.xty, pr.sval = dptr(o.center), dptr(o.scale), dptr(o.xty), dptr(o.sval)
    pr.sptr = o.sptr.ctypes.data_as(C.POINTER(C.c_int64))
    pr.sidx = o.sidx.ctypes.data_as(C.POINTER(C.c_int32))
    pr.rec, pr.rec_bytes_cap = o.rec.ctypes.data, o.rec.size
    pr.ovf, pr.ovf_bytes_cap = o.ovf.ctypes.data, o.ovf.size
    check(_lib.load().sgdnet_setup_probe_sparse(C.byref(csc), int(bool(standardize)), dptr(ymap), cols, dptr(y), y_rows,
                                                int(rec_align), int(device), C.byref(pr)))
    for name in ("max_mean_sq", "max_sqnorm", "rec_stride", "rec_cap", "rec_val_off", "n_ovf", "l_f"):
        setattr(o, name, getattr(pr, name))
    o.sidx, o.sval = o.sidx[:nnz], o.sval[:nnz]
    o.rec = o.rec[:n * o.rec_stride].copy()
    o.ovf = o.ovf[:o.n_ovf * OVF_STRIDE].copy()
    return o


def setup_probe_dense(x, ymap, standardize=True, sample_stride=1, sample_m=0, device=0):
    """x: (n, p) array; ymap: (n, cols).  Returns center, scale, max_mean_sq, xty (p, cols), xt (n, p): the
    standardised matrix as the device holds it sample-major, max_sqnorm, sample (sample_m, p): dense_sample_rows."""
    x = np.asfortranarray(np.asarray(x, dtype=np.float64))
    n, p = x.shape
    ymap = np.asfortranarray(np.asarray(ymap, dtype=np.float64).reshape(n, -1))
    cols = ymap.shape[1]
    o = SimpleNamespace(center=np.empty(p), scale=np.empty(p), xty=np.empty((p, cols), order="F"),
                        xt=np.empty((n, p)), sample=np.empty((sample_m, p), order="F"))
    pr = _lib.SetupProbe()
    pr.center, pr.scale, pr.xty, pr.xt = dptr(o.center), dptr(o.scale), dptr(o.xty), dptr(o.xt)
    if sample_m:
        pr.sample = dptr(o.sample)
    check(_lib.load().sgdnet_setup_probe_dense(dptr(x), n, p, int(bool(standardize)), dptr(ymap), cols, int(sample_stride),
                                               int(sample_m), int(device), C.byref(pr)))
    o.max_mean_sq, o.max_sqnorm = pr.max_mean_sq, pr.max_sqnorm
    return o


NEWTON_REC = ("loss", "half_sq", "abs", "change", "size", "sweeps", "converged", "negligible")


def newton_probe(x, y, scale, u_cur, u, t=0.5, centre=True, l2=0.0, l1=0.0, ridge=False, fit_intercept=True,
                 max_sweeps=1000, tol=1e-7, device=0):
    """One outer step of Newton mode, pass by pass (sgdnet_newton_probe_dense, or _sparse for a scipy.sparse x, whose CSC
    slots go to the library as they are).  scale: (p,); u_cur, u: (p + 1,).  Returns mean; pub_u, pub_a, pub_rec and
    blend_u, blend_a, blend_rec (u published as it is, and blended with u_cur at t; the records are dicts of half_sq, abs,
    change, size); v, r, loss, V, R (the state pass at u); M ((p + 2, p + 2), defined for j <= k and at the corners);
    cd_u, cd_a, cd_rec (the inner solve on M about u_cur; a dict of all eight fields)."""
    sparse = hasattr(x, "tocsc")
    if sparse:
        n, p = x.shape
        colptr = np.ascontiguousarray(x.indptr, dtype=np.int32)
        rowidx = np.ascontiguousarray(x.indices, dtype=np.int32)
        vals = np.ascontiguousarray(x.data, dtype=np.float64)
        csc = _lib.Csc()
        csc.n_rows, csc.n_cols = n, p
        csc.colptr = colptr.ctypes.data_as(C.POINTER(C.c_int32))
        csc.rowidx = rowidx.ctypes.data_as(C.POINTER(C.c_int32))
        csc.values = dptr(vals)
    else:
        x = np.asfortranarray(np.asarray(x, dtype=np.float64))
        n, p = x.shape
    ins = [np.ascontiguousarray(a, dtype=np.float64).reshape(k) for a, k in ((y, n), (scale, p), (u_cur, p + 1), (u, p + 1))]
    o = SimpleNamespace(mean=np.empty(p), v=np.empty(n), r=np.empty(n), M=np.empty((p + 2, p + 2)),
                        **{f"{s}_{w}": np.empty(p + 1) for s in ("pub", "blend", "cd") for w in ("u", "a")})
    pr = _lib.NewtonProbe()
    pr.y, pr.scale, pr.u_cur, pr.u = (dptr(a) for a in ins)
    pr.t, pr.l2, pr.l1, pr.tol = float(t), float(l2), float(l1), float(tol)
    pr.centre, pr.ridge, pr.fit_intercept, pr.max_sweeps = int(bool(centre)), int(bool(ridge)), int(bool(fit_intercept)), int(max_sweeps)
    for name in ("mean", "v", "r", "M", "pub_u", "pub_a", "blend_u", "blend_a", "cd_u", "cd_a"):
        setattr(pr, name, dptr(getattr(o, name)))
    L = _lib.load()
    check(L.sgdnet_newton_probe_sparse(C.byref(csc), int(device), C.byref(pr)) if sparse else
          L.sgdnet_newton_probe_dense(dptr(x), n, p, int(device), C.byref(pr)))
    o.loss, o.V, o.R = pr.loss, pr.V, pr.R
    o.pub_rec = dict(zip(NEWTON_REC[1:5], pr.pub_rec))
    o.blend_rec = dict(zip(NEWTON_REC[1:5], pr.blend_rec))
    o.cd_rec = dict(zip(NEWTON_REC, pr.cd_rec))
    return o


def mnewton_probe(x, y, K, scale, u_cur, u, t=0.5, centre=True, l2=0.0, l1=0.0, ridge=False, fit_intercept=True,
                  max_sweeps=1000, tol=1e-7, width=0, device=0):
    """One outer step of multinomial Newton mode, pass by pass (sgdnet_mnewton_probe; dense x only).  y: n class codes
    0 .. K - 1; scale: (p,); u_cur, u: (K, p + 1) or flat, coordinate (k, j) at k (p + 1) + j, j = p the intercept.
    width: lanes of the inner solve, 64 or 256 (0: the rule a fit follows).  Returns mean; pub_u, pub_a, pub_rec and
    blend_u, blend_a, blend_rec (u published as it is, and blended with u_cur at t; flat, Q = K (p + 1); the records are
    dicts of half_sq, abs, change, size); mu (n, K) and loss (the state pass at u); M (K (K + 1) / 2, p + 2, p + 2), the
    class pairs (k, l), k <= l, row by row of the upper triangle (include/sgdnet_hip.h says which entries are defined);
    cd_u, cd_a, cd_rec (the inner solve on M about u_cur; a dict of all eight fields)."""
    x = np.asfortranarray(np.asarray(x, dtype=np.float64))
    n, p = x.shape
    K = int(K)
    Q, pairs = max(K, 0) * (p + 1), max(K, 0) * (max(K, 0) + 1) // 2
    ins = [np.ascontiguousarray(a, dtype=np.float64).reshape(k) for a, k in ((y, n), (scale, p), (u_cur, Q), (u, Q))]
    o = SimpleNamespace(mean=np.empty(p), mu=np.empty((n, max(K, 0)), order="F"), M=np.empty((pairs, p + 2, p + 2)),
                        **{f"{s}_{w}": np.empty(Q) for s in ("pub", "blend", "cd") for w in ("u", "a")})
    pr = _lib.MNewtonProbe()
    pr.y, pr.scale, pr.u_cur, pr.u = (dptr(a) for a in ins)
    pr.K, pr.width = K, int(width)
    pr.t, pr.l2, pr.l1, pr.tol = float(t), float(l2), float(l1), float(tol)
    pr.centre, pr.ridge, pr.fit_intercept, pr.max_sweeps = int(bool(centre)), int(bool(ridge)), int(bool(fit_intercept)), int(max_sweeps)
    for name in ("mean", "mu", "M", "pub_u", "pub_a", "blend_u", "blend_a", "cd_u", "cd_a"):
        setattr(pr, name, dptr(getattr(o, name)))
    check(_lib.load().sgdnet_mnewton_probe(dptr(x), n, p, int(device), C.byref(pr)))
    o.loss = pr.loss
    o.pub_rec = dict(zip(NEWTON_REC[1:5], pr.pub_rec))
    o.blend_rec = dict(zip(NEWTON_REC[1:5], pr.blend_rec))
    o.cd_rec = dict(zip(NEWTON_REC, pr.cd_rec))
    return o


def wnewton_probe(x, y, scale, u_cur, u, t=0.5, centre=True, l2=0.0, l1=0.0, ridge=False, fit_intercept=True,
                  max_sweeps=1000, tol=1e-7, width=0, device=0):
    """One outer step of wide Newton mode, pass by pass (sgdnet_wnewton_probe; dense x only).  The arguments and the fields
    of newton_probe; width: lanes of the list solve, 256 or 1024 (0: the rule a fit follows).  Added: ld; H (p + 1, ld):
    row j is column j of the matrix as wide_scale_kernel wrote it, H[j, k] = H_kj, the zero pad k >= p + 1 included; Hd
    (p + 1,): its diagonal; q (p + 1,): the right-hand side.  They are copied between the scale kernel and the solve."""
    x = np.asfortranarray(np.asarray(x, dtype=np.float64))
    n, p = x.shape
    P = p + 1
    ld = (P + 15) // 16 * 16
    ins = [np.ascontiguousarray(a, dtype=np.float64).reshape(k) for a, k in ((y, n), (scale, p), (u_cur, P), (u, P))]
    o = SimpleNamespace(mean=np.empty(p), v=np.empty(n), r=np.empty(n), M=np.empty((p + 2, p + 2)),
                        H=np.empty((P, ld)), Hd=np.empty(P), q=np.empty(P),
                        **{f"{s}_{w}": np.empty(P) for s in ("pub", "blend", "cd") for w in ("u", "a")})
    pr = _lib.WNewtonProbe()
    pr.y, pr.scale, pr.u_cur, pr.u = (dptr(a) for a in ins)
    pr.width = int(width)
    pr.t, pr.l2, pr.l1, pr.tol = float(t), float(l2), float(l1), float(tol)
    pr.centre, pr.ridge, pr.fit_intercept, pr.max_sweeps = int(bool(centre)), int(bool(ridge)), int(bool(fit_intercept)), int(max_sweeps)
    for name in ("mean", "v", "r", "M", "H", "Hd", "q", "pub_u", "pub_a", "blend_u", "blend_a", "cd_u", "cd_a"):
        setattr(pr, name, dptr(getattr(o, name)))
    check(_lib.load().sgdnet_wnewton_probe(dptr(x), n, p, int(device), C.byref(pr)))
    if pr.ld != ld:
        raise RuntimeError(f"sgdnet_wnewton_probe: leading dimension {pr.ld}, the binding allocated {ld}")
    o.ld = pr.ld
    o.loss, o.V, o.R = pr.loss, pr.V, pr.R
    o.pub_rec = dict(zip(NEWTON_REC[1:5], pr.pub_rec))
    o.blend_rec = dict(zip(NEWTON_REC[1:5], pr.blend_rec))
    o.cd_rec = dict(zip(NEWTON_REC, pr.cd_rec))
    return o


def wmnewton_probe(x, y, K, scale, u_cur, u, t=0.5, centre=True, l2=0.0, l1=0.0, ridge=False, fit_intercept=True,
                   max_sweeps=1000, tol=1e-7, width=0, device=0):
    """One outer step of wide multinomial Newton mode, pass by pass (sgdnet_wmnewton_probe; dense x only).  The arguments and
    the fields of mnewton_probe; width: lanes of the list solve, 256 or 1024 (0: the rule a fit follows).  Added: ld; H
    (Q, ld): row c is column c of the joint matrix as mnewton_wide_scale_kernel wrote it, the zero pad included; Hd (Q,):
    its diagonal; q (Q,): the right-hand side.  They are copied between the scale kernel and the solve."""
    x = np.asfortranarray(np.asarray(x, dtype=np.float64))
    n, p = x.shape
    K = int(K)
    Q, pairs = max(K, 0) * (p + 1), max(K, 0) * (max(K, 0) + 1) // 2
    ld = (Q + 15) // 16 * 16
    ins = [np.ascontiguousarray(a, dtype=np.float64).reshape(k) for a, k in ((y, n), (scale, p), (u_cur, Q), (u, Q))]
    o = SimpleNamespace(mean=np.empty(p), mu=np.empty((n, max(K, 0)), order="F"), M=np.empty((pairs, p + 2, p + 2)),
                        H=np.empty((Q, ld)), Hd=np.empty(Q), q=np.empty(Q),
                        **{f"{s}_{w}": np.empty(Q) for s in ("pub", "blend", "cd") for w in ("u", "a")})
    pr = _lib.WMNewtonProbe()
    pr.y, pr.scale, pr.u_cur, pr.u = (dptr(a) for a in ins)
    pr.K, pr.width = K, int(width)
    pr.t, pr.l2, pr.l1, pr.tol = float(t), float(l2), float(l1), float(tol)
    pr.centre, pr.ridge, pr.fit_intercept, pr.max_sweeps = int(bool(centre)), int(bool(ridge)), int(bool(fit_intercept)), int(max_sweeps)
    for name in ("mean", "mu", "M", "H", "Hd", "q", "pub_u", "pub_a", "blend_u", "blend_a", "cd_u", "cd_a"):
        setattr(pr, name, dptr(getattr(o, name)))
    check(_lib.load().sgdnet_wmnewton_probe(dptr(x), n, p, int(device), C.byref(pr)))
    if pr.ld != ld:
        raise RuntimeError(f"sgdnet_wmnewton_probe: leading dimension {pr.ld}, the binding allocated {ld}")
    o.ld = pr.ld
    o.loss = pr.loss
    o.pub_rec = dict(zip(NEWTON_REC[1:5], pr.pub_rec))
    o.blend_rec = dict(zip(NEWTON_REC[1:5], pr.blend_rec))
    o.cd_rec = dict(zip(NEWTON_REC, pr.cd_rec))
    return o


def _csc_of(x):
    """(Csc, the arrays it points into): the CSC slots of a scipy.sparse x as they are (row order within a column included)"""
    n, p = x.shape
    keep = (np.ascontiguousarray(x.indptr, dtype=np.int32), np.ascontiguousarray(x.indices, dtype=np.int32),
            np.ascontiguousarray(x.data, dtype=np.float64))
    csc = _lib.Csc()
    csc.n_rows, csc.n_cols = n, p
    csc.colptr = keep[0].ctypes.data_as(C.POINTER(C.c_int32))
    csc.rowidx = keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    csc.values = dptr(keep[2])
    return csc, keep


def _cov_fields(handle, shapes):
    """the named arrays of a sgdnet_cov_probe, copied and shaped; the handle is freed"""
    L = _lib.load()
    o = SimpleNamespace()
    try:
        for name, shape in shapes.items():
            data = C.POINTER(C.c_double)()
            count = L.sgdnet_cov_probe_field(handle, name.encode(), C.byref(data))
            if count < 0:
                continue
            a = np.ctypeslib.as_array(data, shape=(count,)).copy() if count else np.empty(0)
            if name == "ld":
                o.ld = int(a[0])
                continue
            if name in ("sweeps", "unconverged", "max_iter"):
                a = a.astype(np.int64)
            want = shape(o) if callable(shape) else shape
            if int(np.prod(want)) != count:
                raise RuntimeError(f"sgdnet_cov_probe: field {name} has {count} doubles, the binding expected {want}")
            setattr(o, name, a.reshape(want))
    finally:
        L.sgdnet_cov_probe_free(handle)
    return o


def covariance_probe(x, y, scale, mix, lambda_, *, wide=False, multi=None, centre=True, device=0, tol=1e-7, max_sweeps=1000, width=0):
    """One fit of the covariance family stage by stage (sgdnet_covariance_path_probe).  x: (n, p) array or scipy.sparse CSC (its
    slots go to the library as they are); y: (n,) or (n, K) as the driver would hand it over; scale: (p,); multi: the
    K-response form (default: K > 1).  Returns mu, M (P, P) with P = p + K, and c (p, K) (narrow) or ld, S (p, ld), Sd (p,),
    ct (p, K) (wide); include/sgdnet_hip.h says which entries of M are defined.  The path kernel ran with tol and
    max_sweeps in a workgroup of `width` lanes (0: the rule a fit follows) and left W, G (L, p, K), sweeps, unconverged (L,
    integers), and tol, max_iter as it got them."""
    sparse = hasattr(x, "tocsc")
    n, p = x.shape
    y = np.asfortranarray(np.asarray(y, dtype=np.float64).reshape(n, -1))
    K = y.shape[1]
    multi = K > 1 if multi is None else bool(multi)
    scale = np.ascontiguousarray(scale, dtype=np.float64).reshape(p)
    lam = np.ascontiguousarray(lambda_, dtype=np.float64).reshape(-1)
    handle = C.c_void_p()
    L = _lib.load()
    tail = (dptr(y), K, dptr(scale), int(bool(centre)), int(bool(wide)), int(multi), float(mix), lam.size, dptr(lam), int(device),
            float(tol), int(max_sweeps), int(width), C.byref(handle))
    if sparse:
        csc, keep = _csc_of(x)
        check(L.sgdnet_covariance_path_probe(None, C.byref(csc), n, p, *tail))
    else:
        xd = np.asfortranarray(np.asarray(x, dtype=np.float64))
        check(L.sgdnet_covariance_path_probe(dptr(xd), None, n, p, *tail))
    P, nl = p + K, lam.size
    return _cov_fields(handle, {"ld": (1,), "mu": (P if multi else p + 2,), "M": (P, P), "c": (p, K), "S": lambda o: (p, o.ld),
                                "Sd": (p,), "ct": (p, K), "W": (nl, p, K), "G": (nl, p, K), "sweeps": (nl,), "unconverged": (nl,),
                                "tol": (1,), "max_iter": (1,)})


def cv_covariance_probe(x, y, fold, n_groups, alphas, lambdas, *, train_on="fold", wide=False, intercept=True, standardize=True,
                        standardize_response=False, family=None, n_classes=None, maxit=1000, thresh=1e-7, n_gpus=0, debug=0,
                        device=0):
    """A cross-validation of the covariance family stage by stage (sgdnet_cv_covariance_probe): the arguments of
    sgdnet_cv_*covariance_*.  fold: group ids 0 .. n_groups - 1; alphas: (A,); lambdas: (A, L).  y (n,): gaussian; (n, K):
    mgaussian (family and n_classes override what y's shape says, for the refusals).  Returns mu, Mg (G, Pa, Pa), total
    (Pa, Pa; train_on = "rest"), scale (G, p), mean (G, p + K), tstat (3, G), pen_a and pen_b (A, G, L), ridge (A, G), and Mt
    (narrow) or ld, s, d (G, p + K), ysd (G, K; mgaussian), S (G, p, ld), Sd (G, p), ct (G, p, K) (wide); and what the path
    kernel wrote: W, G (A, G, L, p, K), sweeps, unconverged (A, G, L; integers), with tol and max_iter as it got them."""
    sparse = hasattr(x, "tocsc")
    n, p = x.shape
    y = np.asarray(y, dtype=np.float64)
    multi = y.ndim == 2
    y = np.asfortranarray(y.reshape(n, -1))
    K = y.shape[1]
    fold = np.ascontiguousarray(fold, dtype=np.int32).reshape(-1)
    alphas = np.ascontiguousarray(np.atleast_1d(alphas), dtype=np.float64)
    lam = np.ascontiguousarray(np.asarray(lambdas, dtype=np.float64).reshape(alphas.size, -1))
    A, nl, G = alphas.size, lam.shape[1], int(n_groups)
    ctl = _lib.Control()
    ctl.family = _lib.FAMILIES[family or ("mgaussian" if multi else "gaussian")]
    ctl.intercept, ctl.standardize, ctl.standardize_response = int(intercept), int(standardize), int(bool(standardize_response))
    ctl.max_iter, ctl.tol, ctl.n_lambda, ctl.n_classes = int(maxit), float(thresh), nl, int(K if n_classes is None else n_classes)
    ctl.n_gpus, ctl.debug, ctl.device = int(n_gpus), int(debug), int(device)
    handle = C.c_void_p()
    L = _lib.load()
    tail = (dptr(y), fold.ctypes.data_as(C.POINTER(C.c_int32)), G, int(train_on == "rest"), C.byref(ctl), int(bool(wide)), A,
            dptr(alphas), dptr(lam), C.byref(handle))
    if sparse:
        csc, keep = _csc_of(x)
        check(L.sgdnet_cv_covariance_probe(None, C.byref(csc), n, p, *tail))
    else:
        xd = np.asfortranarray(np.asarray(x, dtype=np.float64))
        check(L.sgdnet_cv_covariance_probe(dptr(xd), None, n, p, *tail))
    Pa = p + K + 1
    o = _cov_fields(handle, {"ld": (1,), "mu": (p + 2 * K if multi else p + 2,), "Mg": (G, Pa, Pa), "total": (Pa, Pa),
                             "Mt": (G, p, p + K) if multi else (G, p + 1, p + 1), "scale": (G, p), "mean": (G, p + K), "tstat": (3, G),
                             "pen_a": (A, G, nl), "pen_b": (A, G, nl), "ridge": (A, G), "s": (G, p + K), "d": (G, p + K), "ysd": (G, K),
                             "S": lambda o: (G, p, o.ld), "Sd": (G, p), "ct": (G, p, K), "W": (A, G, nl, p, K), "G": (A, G, nl, p, K),
                             "sweeps": (A, G, nl), "unconverged": (A, G, nl), "tol": (1,), "max_iter": (1,)})
    return o
