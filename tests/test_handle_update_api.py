"""refresh_matrix and the re-keying of the handle cache on CPU tensors, and the header's declarations (no GPU needed).

The cache key of a matrix is (layout, shape, device, dtype) + one part key per component tensor; a part key's field 1 is a version
counter -- the SPARSE tensor's, whichever component is asked, so an in-place change of the values moves it in all three part keys.
refresh_matrix(A) looks for the entry that equals A's key in everything but those counters; refresh_matrix(A, like=B) demands the
index tensors' part keys equal but for the counter -- identity, never contents."""
import os
import re

import pytest
import torch

from pytorch_sparse_solver import _hipk
from pytorch_sparse_solver import module_a as MA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _csr(n=6, scale=1.0):
    crow = torch.arange(n + 1, dtype=torch.int64)
    col = torch.arange(n, dtype=torch.int64)
    return torch.sparse_csr_tensor(crow, col, scale * torch.arange(1, n + 1, dtype=torch.float64), size=(n, n))


def test_refresh_matrix_is_exported_and_returns_false_without_a_cached_handle():
    assert "refresh_matrix" in MA.__all__ and callable(MA.refresh_matrix)
    _hipk.clear_cache()
    A = _csr()
    assert MA.refresh_matrix(A) is False
    A.values().mul_(2)
    assert MA.refresh_matrix(A) is False
    B = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values() * 3, size=A.shape)
    assert MA.refresh_matrix(B, like=A) is False
    assert _hipk.cache_info()[0] == 0


def test_refresh_matrix_refuses_what_is_not_the_same_pattern_object():
    A = _csr()
    with pytest.raises(ValueError, match="index tensors of its own"):
        MA.refresh_matrix(_csr(scale=2.0), like=A)                 # equal contents, tensors of its own
    B = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices().clone(), A.values() * 3, size=A.shape)
    with pytest.raises(ValueError, match="index tensors of its own"):
        MA.refresh_matrix(B, like=A)
    with pytest.raises(ValueError, match="shape"):
        MA.refresh_matrix(_csr(7), like=A)
    with pytest.raises(ValueError, match="dtype"):
        MA.refresh_matrix(A.to(torch.float32), like=A)
    for bad in (A.to_dense(), A.to_sparse_coo(), "A"):
        with pytest.raises(ValueError, match="CSR"):
            MA.refresh_matrix(bad)
        with pytest.raises(ValueError, match="CSR"):
            MA.refresh_matrix(A, like=bad)


def test_the_key_of_an_in_place_change_differs_in_the_version_counters_alone():
    A = _csr()
    k0 = _hipk._cache_key(A)
    assert _hipk._same_but_version(k0, k0)
    A.values().mul_(2)
    k1 = _hipk._cache_key(A)
    assert k1 != k0 and _hipk._same_but_version(k0, k1)
    assert all(a[1] + 1 == b[1] and _hipk._no_version(a) == _hipk._no_version(b) for a, b in zip(k0[4:], k1[4:]))
    assert not _hipk._same_but_version(k1, _hipk._cache_key(_csr()))                     # other storage
    assert not _hipk._same_but_version(k1, _hipk._cache_key(A.to(torch.float32)))
    assert not _hipk._same_but_version(k1, _hipk._cache_key(torch.sparse_csr_tensor(A.crow_indices(), A.col_indices()[:5], A.values()[:5],
                                                                                    size=A.shape)))
    B = torch.sparse_csr_tensor(A.crow_indices(), A.col_indices(), A.values() * 3, size=A.shape)
    kb, ka = _hipk._cache_key(B), _hipk._cache_key(A)              # what like= compares: the index tensors' part keys
    assert [_hipk._no_version(p) for p in kb[4:6]] == [_hipk._no_version(p) for p in ka[4:6]] and _hipk._no_version(kb[6]) != _hipk._no_version(ka[6])
    assert kb[4][1] == 0 and ka[4][1] == 1                         # B counts its own writes


def test_the_header_declares_the_update_entry_points():
    with open(os.path.join(ROOT, "include", "hipk.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+hipk_csr_update_values\(hipk_csr_t h, const void \*val_dev, hipk_stream_t stream\);", text)
    assert re.search(r"\bint\s+hipk_last_csr_update_kind\(void\);", text)
    assert "#define HIPK_VERSION 300" in text
    assert "unchanged until hipk_csr_destroy" not in text and "hipk_csr_update_values is called" in text
    assert {"hipk_csr_update_values", "hipk_last_csr_update_kind"} <= set(_hipk.SYMBOLS)
