"""A CPU mirror of BiCGStab with M = blockdiag(binv) in both storage dtypes: what hipk_pbicgstab_solve_cb computes with a
`BlockJacobiPreconditioner` as its callable, and what hipk_bi_bjbatch_kernel computes per system (csrc/hipk_batch_bj.hip).

It is `bicgstab_impl` of oracle/krylov_oracle.c with two changes -- phat = M p and shat = M s come from the block apply instead of
the row scale, and the final test is t = b - A x, z = M t, residual_norm^2 = the PLAIN dot <z,z> -- composed from the oracle's own
pieces: spmv, the plain and the tiled dot, orc_block_jacobi_apply.  The element-wise chains are numpy operations in the storage
dtype, one rounding each, in the order the C source writes them; the scalars are doubles.

CG needs no mirror: the oracle has orc_pcg_blockjacobi in both dtypes (`pcg_blockjacobi` below picks the dtype)."""
import ctypes

import numpy as np

EPS = {np.float64: 2.220446049250313e-16, np.float32: 1.1920928955078125e-07}


def _kit(O, dt):
    """spmv, dot, dot_tiled, apply of the oracle for storage dtype dt."""
    if dt == np.float64:
        return O.spmv, O.dot, O.dot_tiled, O.block_jacobi_apply
    fp = ctypes.POINTER(ctypes.c_float)
    fn = O.lib().orc32_block_jacobi_apply
    fn.argtypes = [ctypes.c_int64, ctypes.c_int, fp, fp, fp]

    def apply32(binv, v):
        binv, v = np.ascontiguousarray(binv, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        out = np.empty_like(v)
        fn(v.size, int(binv.shape[1]), binv.ctypes.data_as(fp), v.ctypes.data_as(fp), out.ctypes.data_as(fp))
        return out

    return O.spmv32, O.dot32, O.dot_tiled32, apply32


def block_apply(O, binv, v, dtype):
    return _kit(O, np.dtype(dtype).type)[3](binv, v)


def _norm(v):
    return float(np.sqrt(np.float64(0.0) if v < 0.0 else np.float64(v)))


def _tmax(a, b):
    return float("nan") if (a != a or b != b) else (a if a > b else b)


def bicgstab_block(O, crow, col, val, binv, b, x0=None, tol=1e-5, atol=0.0, maxiter=None, dtype=np.float64):
    """-> oracle.OracleResult (and `.exit_early`).  binv: (ceil(n / bs), bs, bs)."""
    dt = np.dtype(dtype).type
    spmv, dot, dot_tiled, apply = _kit(O, dt)
    eps = EPS[dt]
    val, b = np.ascontiguousarray(val, dtype=dt), np.ascontiguousarray(b, dtype=dt)
    binv = np.ascontiguousarray(binv, dtype=dt)
    n = b.size
    x = np.zeros(n, dtype=dt) if x0 is None else np.array(x0, dtype=dt, copy=True)
    maxiter = 10 * n if maxiter is None or maxiter < 0 else int(maxiter)
    f8 = np.float64
    with np.errstate(all="ignore"):
        bs = f8(dot(b, b))
        tolf, atolf = np.float32(tol), np.float32(atol)
        a2, a3 = f8(tolf * tolf) * bs, f8(atolf * atolf)
        atol2 = a2 if a2 > a3 else a3
        r = spmv(crow, col, val, x, b)
        matvecs = 1
        rhat, p, q = r.copy(), r.copy(), r.copy()
        alpha = omega = rho = f8(1.0)
        rs = f8(0.0)
        k, code, early = 0, 0, False
        rs_next = f8(dot_tiled(r, r))
        rho_next = rs_next
        while k < maxiter:
            rs = rs_next
            if rs <= atol2:
                break
            rho_new = rho_next
            if abs(rho_new) < eps * abs(rho):
                code = -10
                break
            beta = rho_new / rho * alpha / omega
            t1 = dt(omega) * q
            t2 = p - t1
            t3 = dt(beta) * t2
            p = r + t3
            phat = apply(binv, p)
            q = spmv(crow, col, val, phat)
            matvecs += 1
            alpha_new = rho_new / f8(dot_tiled(rhat, q))
            if abs(alpha_new) < eps:
                code = -11
                break
            m = dt(alpha_new) * q
            s = r - m
            shat = apply(binv, s)
            exit_early = f8(dot(s, s)) < atol2
            t = spmv(crow, col, val, shat)
            matvecs += 1
            tt = f8(dot_tiled(t, t))
            omega_new = f8(0.0) if abs(tt) < eps else f8(dot_tiled(s, t)) / tt
            if abs(omega_new) < eps and not exit_early:
                code = -11
                break
            m0 = dt(alpha_new) * phat
            if exit_early:
                x = x + m0
                r = s
            else:
                m1 = dt(omega_new) * shat
                m2 = m0 + m1
                x = x + m2
                m3 = dt(omega_new) * t
                r = s - m3
            rs_next = f8(dot(r, r))
            rho_next = f8(dot(rhat, r))
            rho, alpha, omega = rho_new, alpha_new, omega_new
            k += 1
            if exit_early:
                early = True
                break
        z = apply(binv, spmv(crow, col, val, x, b))
        b_norm = _norm(bs)
        residual_norm = _norm(f8(dot(z, z)))
        x_norm = _norm(f8(dot(x, x)))
    threshold = _tmax(float(np.float32(tol)) * b_norm, float(np.float32(atol)))
    info = -1 if (x_norm != x_norm or residual_norm > threshold) else 0
    assert x.dtype == dt
    res = O.OracleResult(x=x, info=info, iterations=k, matvecs=matvecs + 1, breakdown=code, b_norm=b_norm,
                         residual_norm=residual_norm, x_norm=x_norm, threshold=threshold, recurrence_rs=float(rs))
    res.exit_early = early          # the loop left through `exit_early` (TSL:924): the case tables want to see that exit taken
    return res


def pcg_blockjacobi(O, crow, col, val, binv, b, x0=None, tol=1e-5, atol=0.0, maxiter=None, dtype=np.float64):
    """orc_pcg_blockjacobi / orc32_pcg_blockjacobi -> oracle.OracleResult."""
    if np.dtype(dtype) == np.float64:
        return O.pcg_blockjacobi(crow, col, val, binv, b, x0, tol=tol, atol=atol, maxiter=maxiter)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    fn = O.lib().orc32_pcg_blockjacobi
    fn.argtypes = [ctypes.c_int64, ip, ip, fp, ctypes.c_int, fp, fp, fp, ctypes.c_double, ctypes.c_double, ctypes.c_int64,
                   ctypes.POINTER(O._Stats)]
    crow, col, val, b, x = O._prep32(crow, col, val, b, x0)
    binv = np.ascontiguousarray(binv, dtype=np.float32)
    st = O._Stats()
    fn(b.size, O._i(crow), O._i(col), O._f(val), int(binv.shape[1]), O._f(binv), O._f(b), O._f(x), float(tol), float(atol),
       -1 if maxiter is None else int(maxiter), ctypes.byref(st))
    return O._result(x, st)
