"""CPU: nn.dense_to_csr, the one place where the item-item models turn a dense batch into the CSR their scores
kernels read, against scipy.sparse.csr_matrix on host tensors."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from recoder_amd.nn import dense_to_csr

N = 70


def _check(dense, items):
  """dense [B, C] f32 numpy, items None or the C catalogue ids of its columns."""
  B, C = dense.shape
  full = np.zeros((B, N), np.float32)
  full[:, np.arange(C) if items is None else items] = dense
  want = sp.csr_matrix(full)
  want.sort_indices()
  got = dense_to_csr(torch.from_numpy(dense), None if items is None else torch.from_numpy(items), N)
  assert got.shape == (B, N)
  assert got.indptr.dtype == torch.int64 and got.indices.dtype == torch.int32 and got.data.dtype == torch.float32
  assert got.indices.is_contiguous() and got.data.is_contiguous()
  assert np.array_equal(got.indptr.numpy(), want.indptr)
  nnz = int(want.nnz)
  assert got.data.numel() == nnz and np.array_equal(got.data.numpy(), want.data)
  if nnz:
    assert np.array_equal(got.indices.numpy(), want.indices)
    for u in range(B):
      row = got.indices.numpy()[want.indptr[u]:want.indptr[u + 1]]
      assert np.all(np.diff(row) > 0)
  else:
    assert got.indices.numel() == 1            # (the placeholder: the kernels take a non-null pointer)
  return got


def _batch(C, seed):
  rng = np.random.RandomState(seed)
  dense = np.where(rng.rand(3, C) < 0.3, rng.randint(1, 9, size=(3, C)) * 0.25 + 0.125, 0).astype(np.float32)
  dense[1] = 0                                 # (an empty middle row)
  assert (dense[0] != 0).sum() > 2 and (dense[2] != 0).sum() > 2 and len(np.unique(dense)) > 3
  return dense


@pytest.mark.parametrize("dtype", [np.int64, np.int32])
def test_a_permuted_subset_of_the_catalogue_with_an_empty_row(dtype):
  items = np.random.RandomState(1).permutation(N)[:41].astype(dtype)
  assert np.any(np.diff(items) < 0) and np.any(np.diff(items) > 0)
  got = _check(_batch(41, 2), items)
  assert got.indptr[1] == got.indptr[2]


def test_all_columns_without_input_items():
  _check(_batch(N, 3), None)


@pytest.mark.parametrize("items", [None, np.array([69, 3, 40, 0], np.int64)])
def test_an_all_zero_batch_keeps_a_one_element_placeholder(items):
  got = _check(np.zeros((3, N if items is None else 4), np.float32), items)
  assert got.indptr.tolist() == [0, 0, 0, 0]
