"""Dtype-aware mirror of the step API of include/hipk.h (TEST CODE): one method per entry point, plain numpy plus the oracle's
primitives, following the arithmetic written in the kernels of csrc/hipk_cg.hip call by call.

Operands are numpy arrays of the call's dtype T (float64 or float32) and are updated in place, as the device does.  Partial arrays
are float64, 2048 slots; the scalar block is a float64 array whose first 8 words are
    {gamma[0], gamma[1], atol2, bs, res2, xx, stop_it (int64), host_sig (pointer)}
(hipk_cg_scal; the start entry points leave res2 and xx as they find them).  Every product and every sum of the vector updates
is one rounding in T (numpy has no fma); alpha and beta are rounded to T once, from fp64 quotients; chunk partials are the
oracle's (fp32: its fp32 build, where a virtual thread owns 4 elements per step instead of 2) and folds are oracle.reduce_parts.

For fp64 every method agrees bit for bit with tests/dist_cpu_ops.py::OracleOps on the same inputs (tests/test_step_cases.py).
The small methods of the first block are the places a kernel can be subtly wrong; tests/test_step_cases.py overrides them one at
a time to show that the case table tells each such kernel from this one."""
import numpy as np

from oracle import oracle as O

INT64_MAX = np.iinfo(np.int64).max
MAX_PARTS = 2048
BASE_CHUNK = 2048
GAMMA0, GAMMA1, ATOL2, BS, RES2, XX, STOP_IT, HOST_SIG = range(8)
SCAL_WORDS = 8


def vec_width(dtype):
    """Elements of one 16-byte access."""
    return 16 // np.dtype(dtype).itemsize


def stop_word(scal):
    return scal[STOP_IT:STOP_IT + 1].view(np.int64)


def sig_word(scal):
    return scal[HOST_SIG:HOST_SIG + 1].view(np.int64)


def local_chunks(n, ch):
    return (n + ch - 1) // ch


def dot_parts(a, b, ch):
    """Chunk partials of <a, b> in the storage type of a."""
    if a.dtype == np.float32:
        return O.dot_parts_ch32(a, b, ch)
    return O.dot_parts_ch(a, b, ch)


def squared_f32(v):
    """tol -> tol^2 as the host side of the start entry points computes it: the square of the fp32 value, in fp32."""
    f = np.float32(v)
    return float(f * f)


class Mirror:
    # ---- the single decisions of the kernels
    def gamma(self, scal, it):
        return scal[it & 1]

    def fold(self, part, g, n, ch):
        """Partial INPUTS are read from all g slots."""
        return np.float64(O.reduce_parts(part[:g]))

    def coef(self, v, dtype):
        """alpha, beta: the fp64 quotient rounded to T once."""
        return np.dtype(dtype).type(v)

    def mul(self, c, v):
        return c * v

    def touched(self, n, ch, dtype):
        """Which of the n elements a call updates: all of them."""
        return True

    x_reads_new_p = False

    def stop_at_start(self, maxiter, rr0, atol2):
        return bool(maxiter <= 0 or rr0 <= atol2)

    def stop_next(self, it, maxiter, rr, atol2):
        return bool(it + 1 >= maxiter or rr <= atol2)

    def write_parts(self, out, q):
        """Partial OUTPUTS are written to the local slots only."""
        out[:q.size] = q

    def write_start_block(self, scal, gamma0, atol2, bs, stop):
        scal[GAMMA0], scal[GAMMA1], scal[ATOL2], scal[BS] = gamma0, 0.0, atol2, bs
        stop_word(scal)[0] = stop
        sig_word(scal)[0] = 0

    # ---- the entry points
    def _start(self, n, ch, g, scal, gamma0, rr0, bs, src, p, tol, atol, maxiter):
        atol2 = max(squared_f32(tol) * bs, squared_f32(atol))
        np.copyto(p[:n], src[:n], where=self.touched(n, ch, p.dtype))
        self.write_start_block(scal, gamma0, atol2, bs, 0 if self.stop_at_start(maxiter, rr0, atol2) else INT64_MAX)

    def cg_start(self, n, ch, g, scal, part_rr, part_bb, r, p, tol, atol, maxiter):
        gamma0, bs = self.fold(part_rr, g, n, ch), self.fold(part_bb, g, n, ch)
        self._start(n, ch, g, scal, gamma0, gamma0, bs, r, p, tol, atol, maxiter)

    def cgm_start(self, n, ch, g, scal, part_rz, part_rr, part_bb, z, p, tol, atol, maxiter):
        gamma0, rr0, bs = (self.fold(q, g, n, ch) for q in (part_rz, part_rr, part_bb))
        self._start(n, ch, g, scal, gamma0, rr0, bs, z, p, tol, atol, maxiter)

    def _alpha(self, n, ch, g, scal, it, part_pAp, dtype):
        return self.coef(self.gamma(scal, it) / self.fold(part_pAp, g, n, ch), dtype)

    def cg_update(self, n, ch, g, scal, it, part_pAp, Ap, r, part_rr_out):
        if it >= stop_word(scal)[0]:
            return
        with np.errstate(all="ignore"):
            alpha = self._alpha(n, ch, g, scal, it, part_pAp, r.dtype)
            new = r[:n] - self.mul(alpha, Ap[:n])
        np.copyto(r[:n], new, where=self.touched(n, ch, r.dtype))
        self.write_parts(part_rr_out, dot_parts(r[:n], r[:n], ch))

    def cg_xupdate(self, n, ch, g, scal, it, part_pAp, p, x):
        if it >= stop_word(scal)[0]:
            return
        with np.errstate(all="ignore"):
            alpha = self._alpha(n, ch, g, scal, it, part_pAp, x.dtype)
            new = x[:n] + self.mul(alpha, p[:n])
        np.copyto(x[:n], new, where=self.touched(n, ch, x.dtype))

    def _direction(self, n, ch, g, scal, it, maxiter, part_pAp, gamma_new, rr, src, p, x):
        with np.errstate(all="ignore"):
            gamma = self.gamma(scal, it)
            alpha = self._alpha(n, ch, g, scal, it, part_pAp, p.dtype)
            beta = self.coef(gamma_new / gamma, p.dtype)
            sel = self.touched(n, ch, p.dtype)
            p_new = src[:n] + self.mul(beta, p[:n])
            if x is not None:
                x_new = x[:n] + self.mul(alpha, p_new if self.x_reads_new_p else p[:n])
                np.copyto(x[:n], x_new, where=sel)
            np.copyto(p[:n], p_new, where=sel)
        atol2 = scal[ATOL2]
        scal[(it + 1) & 1] = gamma_new
        if self.stop_next(it, maxiter, rr, atol2):
            stop_word(scal)[0] = it + 1

    def cg_direction(self, n, ch, g, scal, it, maxiter, part_pAp, part_rr, r, p, x):
        if it >= stop_word(scal)[0]:
            return
        rr = self.fold(part_rr, g, n, ch)
        self._direction(n, ch, g, scal, it, maxiter, part_pAp, rr, rr, r, p, x)

    def cgm_direction(self, n, ch, g, scal, it, maxiter, part_pAp, part_rz, part_rr, z, p, x):
        if it >= stop_word(scal)[0]:
            return
        gamma_new, rr = self.fold(part_rz, g, n, ch), self.fold(part_rr, g, n, ch)
        self._direction(n, ch, g, scal, it, maxiter, part_pAp, gamma_new, rr, z, p, x)


TRUE = Mirror()
