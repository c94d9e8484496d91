"""Every SpMV kernel instantiation hipk_launch_spmv (csrc/hipk_api.hip) can choose, run through hipk_spmv_ex and pinned to the
oracle, the instantiation asserted from the kernel note (hipk_last_spmv_kernel) -- exactly, template arguments included.

The case table is tests/_spmv_cases.py; tests/test_spmv_cases.py checks without a GPU that it accounts for all 128 hipk_spmv_*
kernels of the gfx950 code object (the nine with the Chebyshev epilogue belong to tests/test_gpu_chebyshev_kernels.py).  Per case:
the switches are set, THEN the handle is created; per mode the note must equal the expected string, y must have the bits of
oracle.spmv / oracle.spmv32 (with bsub for modes >= 4), the chunk partials of <w, y> and <y, y> the bits of the oracle's tiled
dot per reduction chunk (also above n = 20 k, where the other SpMV tests compare them with the plain CSR kernels only), and x, w, b
must be unchanged.  The references are computed once per (matrix, storage type) and are themselves held against np.longdouble
sums with a derived bound (_spmv_inst_worker.py: References.check_against_high_precision).

Switches that a process reads once (HIPK_SPMV_SELL_NO_MODE, HIPK_SPMV_SELL_NO_PAIR, HIPK_SPMV_NO_PLAN_CACHE, and whether
HIPK_SPMV_SELL_CHUNKED is set) run in a child process per setting (_spmv_inst_worker.py), one child at a time."""
import json
import os
import subprocess
import sys

import pytest

import _spmv_cases as C
from _spmv_inst_worker import OnDevice, References, run_case

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_spmv_inst_worker.py")
CHILD_SECONDS = 600       # a child builds up to six references of 2.2 M rows on the CPU and runs up to twelve cases

_held = {}                # (matrix, dtype): (References, OnDevice) -- one at a time of the large ones


def _references(hipk, oracle, matrix, dtype):
    key = (matrix, dtype)
    if key not in _held:
        n = C.MATRICES[matrix][0]
        if n > C.N_SMALL:
            for k in [k for k in _held if C.MATRICES[k[0]][0] > C.N_SMALL]:
                del _held[k]
        ref = References(oracle, matrix, dtype, int(hipk.lib().hipk_chunk_size(n)))
        worst = ref.check_against_high_precision()
        print(f"{matrix} {dtype}: oracle against np.longdouble, largest error / bound {worst:.3f}", flush=True)
        _held[key] = (ref, OnDevice(ref))
    return _held[key]


# in-process cases, cases of one (matrix, storage type) next to each other: its references are computed once
IN_PROCESS = sorted((n for n, c in C.CASES.items() if c["fresh"] is None), key=lambda n: (C.CASES[n]["matrix"], C.CASES[n]["dtype"], n))


@pytest.mark.parametrize("name", IN_PROCESS)
def test_instantiation(hipk, oracle, monkeypatch, name):
    case = C.CASES[name]
    ref, dev = _references(hipk, oracle, case["matrix"], case["dtype"])

    def setenv(k, v):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)

    notes, failures = run_case(hipk, name, ref, dev, setenv)
    print(name, sorted({n[3] for n in notes}), flush=True)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("group", C.FRESH_GROUPS)
def test_fresh_process_group(hipk, tmp_path, group):
    """One child per setting of a switch the library reads once per process; never retried."""
    _held.clear()         # the child holds its own references and device copies
    names = sorted((n for n, c in C.CASES.items() if c["fresh"] == group), key=lambda n: (C.CASES[n]["matrix"], C.CASES[n]["dtype"], n))
    out = str(tmp_path / "result.json")
    try:
        p = subprocess.run([sys.executable, WORKER, group, out] + names, capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"group {group}: the child did not finish in {CHILD_SECONDS} s\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-4000:]}")
    assert p.returncode == 0, f"group {group}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with open(out) as f:
        results = json.load(f)
    failures = []
    for name in names:
        assert name in results, f"group {group}: no result for {name}\n{p.stdout[-2000:]}"
        case, r = C.CASES[name], results[name]
        failures += r["failures"]
        want = [[si, mode, wx, notes[mode]] for si, (_, notes) in enumerate(case["steps"]) for mode, wx in case["runs"]]
        if r["notes"] != want:
            failures.append(f"{name}: notes {r['notes']}, expected {want}")
        print(name, sorted({n[3] for n in r["notes"]}), flush=True)
    assert not failures, "\n".join(failures)
