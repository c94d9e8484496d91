"""The matrix-gradient step (csrc/hipk_vgrad.hip, module_a/matrix_grad.py) on one MI355X, one process; one JSON line per measurement,
also written to `--out` (profiles/matrix_grad_probe.txt), stamped with the library's build id.

1. KERNEL AGAINST THE PRODUCT'S TORCH EXPRESSION on the same arrays: 5-point Poisson 2000^2 (nnz ~ 20 M) in fp64 and fp32,
   `create_variable_diffusion_2d_csr(2000, 2000)` in fp64, and a batch of S = 4096 systems on the 32 x 32 grid (n = 1024).  After a
   warm-up the two are timed `--reps` times in alternation (kernel, torch, kernel, ...), each call between its own pair of device
   events; median and min..max in microseconds.  The torch expression is timed as the product runs it (row indices from crow by
   repeat_interleave, two gathers, a product, a negation) and with the row indices precomputed.  `model_bytes` = nnz (4 + sizeof T)
   + the two vectors, per system; `gbps` = model_bytes / median.  The handle's SpMV on the same matrix (the form its structure analysis
   selects) and the general CSR SpMV (a second handle with the coded forms switched off) are timed the same way for scale.
2. THE GRADIENT STEP'S SHARE OF BACKWARD for cg(tol=1e-6) on Poisson 2000^2 (N = 4 M): forward, backward (adjoint solve + gradient)
   and the gradient kernel alone.
3. THE FORWARD SOLVE with the matrix requiring grad, against the same call through an autograd Function that saves only A (what
   the forward did before it kept x for backward), and against the solve with nothing requiring grad; alternated.

  python tools/matrix_grad_probe.py --out profiles/matrix_grad_probe.txt
  python tools/matrix_grad_probe.py --nx 64 --batch 16 --out profiles/matrix_grad_probe.txt --append     # the launch-bound end
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd"))

import torch  # noqa: E402

DEV = "cuda:0"
LINES = []


def emit(**kw):
    line = json.dumps(kw)
    print(line, flush=True)
    LINES.append(line)


def alternate(fns, reps, warm=3):
    """{name: [microseconds]}: every fn timed `reps` times between its own device events, in alternation, after `warm` calls each."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3)
    return out


def stats(us):
    return {"median_us": round(statistics.median(us), 1), "min_us": round(min(us), 1), "max_us": round(max(us), 1)}


def kernel_vs_torch(name, A, reps):
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import matrix_grad as MG
    A = A.to(DEV)
    h = _hipk.handle_for(A)
    n, nnz, es = A.shape[0], h.nnz, A.values().element_size()
    g = torch.Generator(device=DEV).manual_seed(1)
    lam, x = (torch.randn(n, dtype=A.dtype, device=DEV, generator=g) for _ in range(2))
    crow, col = A.crow_indices(), A.col_indices()
    rows = MG.csr_rows(crow)
    out, y = torch.empty(nnz, dtype=A.dtype, device=DEV), torch.empty(n, dtype=A.dtype, device=DEV)
    hg = _hipk.CsrHandle(crow, col, A.values(), A.shape)      # a second handle kept off the coded forms: the general CSR SpMV
    hg.set_path(True)
    t = alternate({"kernel": lambda: _hipk.csr_grad_values(h, lam, x, out=out),
                   "torch": lambda: MG.grad_values_torch(MG.csr_rows(crow), col, lam, x, A.dtype),
                   "torch_rows_given": lambda: MG.grad_values_torch(rows, col, lam, x, A.dtype),
                   "spmv": lambda: _hipk.spmv(h, x, out=y), "spmv_general": lambda: _hipk.spmv(hg, x, out=y)}, reps)
    assert torch.equal(out, MG.grad_values_torch(rows, col, lam, x, A.dtype)), "kernel and torch expression differ"
    model = nnz * (4 + es) + 2 * n * es
    k = stats(t["kernel"])
    emit(what="kernel_vs_torch", system=name, dtype=str(A.dtype), n=n, nnz=nnz, batch=1, model_bytes=model,
         kernel=k, kernel_gbps=round(model / k["median_us"] / 1e3, 1), torch=stats(t["torch"]), torch_rows_given=stats(t["torch_rows_given"]),
         spmv=stats(t["spmv"]), spmv_path=h.path(), spmv_general=stats(t["spmv_general"]), spmv_general_path=hg.path(), speedup_vs_torch=round(statistics.median(t["torch"]) / k["median_us"], 2),
         speedup_vs_torch_rows_given=round(statistics.median(t["torch_rows_given"]) / k["median_us"], 2), bitwise_equal=True)


def batch_kernel_vs_torch(S, nx, reps):
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import matrix_grad as MG
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr
    A = create_poisson_2d_csr(nx, nx).to(DEV)
    n, nnz = A.shape[0], A.col_indices().numel()
    crow, col = A.crow_indices(), A.col_indices()
    crow32, col32 = crow.to(torch.int32), col.to(torch.int32)
    g = torch.Generator(device=DEV).manual_seed(2)
    Lam, X = (torch.randn((S, n), dtype=torch.float64, device=DEV, generator=g) for _ in range(2))
    out = torch.empty((S, nnz), dtype=torch.float64, device=DEV)
    rows = MG.csr_rows(crow)
    t = alternate({"kernel": lambda: _hipk.batch_grad_values(n, nnz, crow32, col32, Lam, X, out=out),
                   "torch": lambda: MG.grad_values_torch(MG.csr_rows(crow), col, Lam, X, torch.float64),
                   "torch_rows_given": lambda: MG.grad_values_torch(rows, col, Lam, X, torch.float64)}, reps)
    assert torch.equal(out, MG.grad_values_torch(rows, col, Lam, X, torch.float64)), "kernel and torch expression differ"
    model = S * (nnz * 8 + 2 * n * 8) + nnz * 4
    k = stats(t["kernel"])
    emit(what="kernel_vs_torch", system=f"batch poisson {nx}x{nx}", dtype="torch.float64", n=n, nnz=nnz, batch=S, model_bytes=model,
         kernel=k, kernel_gbps=round(model / k["median_us"] / 1e3, 1), torch=stats(t["torch"]), torch_rows_given=stats(t["torch_rows_given"]),
         speedup_vs_torch=round(statistics.median(t["torch"]) / k["median_us"], 2),
         speedup_vs_torch_rows_given=round(statistics.median(t["torch_rows_given"]) / k["median_us"], 2), bitwise_equal=True)


class _SavesOnlyA(torch.autograd.Function):
    """The forward half of the implicit-function wrapper as it was before x was kept: the yardstick of part 3."""

    @staticmethod
    def forward(ctx, A_matrix, b, x):
        ctx.save_for_backward(A_matrix)
        return x

    @staticmethod
    def backward(ctx, grad_output):
        return None, None, None


def backward_share_and_forward(name, A, reps):
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.module_a import cg, get_last_grad_stats, get_last_stats
    from pytorch_sparse_solver.module_a import torch_sparse_linalg as T
    n = A.shape[0]
    Ad = A.to(DEV)
    Ag = Ad.detach().clone().requires_grad_()
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    w = torch.randn(n, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    h = _hipk.handle_for(Ag)
    out = torch.empty(h.nnz, dtype=torch.float64, device=DEV)
    state = {}

    def forward_grad():
        state["x"], state["info"] = cg(Ag, b, tol=1e-6)

    def forward_saves_only_a():
        x, info = T._isolve('cg', Ag.detach(), b, None, 1e-6, 0.0, None, None)
        state["x0"] = _SavesOnlyA.apply(Ag, b, x)

    def forward_plain():
        state["xp"], _ = cg(Ad, b, tol=1e-6)

    t = alternate({"forward_requires_grad": forward_grad, "forward_saves_only_A": forward_saves_only_a, "forward_plain": forward_plain}, reps, warm=2)
    iters = get_last_stats().iterations
    assert torch.equal(state["x"].detach(), state["xp"]) and torch.equal(state["x0"].detach(), state["xp"])
    emit(what="forward_solve", system=name, solver="cg tol=1e-6", n=n, iterations=iters, info=int(state["info"]),
         forward_requires_grad=stats(t["forward_requires_grad"]), forward_saves_only_A=stats(t["forward_saves_only_A"]),
         forward_plain=stats(t["forward_plain"]), x_bitwise_equal=True)

    def fwd_bwd():
        Ag.grad = None
        x, _ = cg(Ag, b, tol=1e-6)
        state["loss"] = (x * w).sum()

    bw, kn = [], []
    for i in range(2 + max(3, reps // 4)):
        fwd_bwd()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        state["loss"].backward()
        e.record()
        e.synchronize()
        x = state["x"]                                  # any vectors of the right length
        a2, e2 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a2.record()
        _hipk.csr_grad_values(h, w, x.detach(), out=out)
        e2.record()
        e2.synchronize()
        if i >= 2:
            bw.append(a.elapsed_time(e) * 1e3)
            kn.append(a2.elapsed_time(e2) * 1e3)
    st = get_last_grad_stats()
    emit(what="backward_share", system=name, solver="cg tol=1e-6", n=n, route=st.route, adjoint_iterations=get_last_stats().iterations,
         backward=stats(bw), gradient_kernel=stats(kn), share=round(statistics.median(kn) / statistics.median(bw), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nx", type=int, default=2000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it (a second run at other sizes)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matrix_grad_probe needs a GPU: nothing here is measured on a CPU")
    from pytorch_sparse_solver import _hipk
    from pytorch_sparse_solver.utils.matrix_utils import create_poisson_2d_csr, create_variable_diffusion_2d_csr
    emit(what="build", build_id=_hipk.lib().hipk_build_id().decode(), device=torch.cuda.get_device_name(0), reps=a.reps, nx=a.nx, batch=a.batch)
    P = create_poisson_2d_csr(a.nx, a.nx)
    kernel_vs_torch(f"poisson {a.nx}x{a.nx}", P, a.reps)
    kernel_vs_torch(f"poisson {a.nx}x{a.nx}", P.to(torch.float32), a.reps)
    kernel_vs_torch(f"variable diffusion {a.nx}x{a.nx}", create_variable_diffusion_2d_csr(a.nx, a.nx), a.reps)
    batch_kernel_vs_torch(a.batch, 32, a.reps)
    _hipk.clear_cache()
    backward_share_and_forward(f"poisson {a.nx}x{a.nx}", P, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
