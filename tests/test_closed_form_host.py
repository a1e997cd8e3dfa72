"""CPU: what the eight closed-form ``Recoder.train_*`` methods share -- the refusal of a model of another class,
a refused call that leaves the Recoder and the model as they were, ``Recoder.train``'s pointers at them -- and
the orientation of the neighbour-list models' ``dense_weights``."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch


def _no_gpu(monkeypatch):
  import recoder_amd.model as model_mod
  from recoder_amd import device

  def no_gpu(*a, **k):
    raise AssertionError("GPU work started")
  monkeypatch.setattr(device, "require_gpu", no_gpu)
  monkeypatch.setattr(model_mod, "require_gpu", no_gpu)
  monkeypatch.setattr(torch.cuda, "mem_get_info", no_gpu)


def _dataset(negative=False):
  from recoder_amd.data import RecommendationDataset
  X = sp.random(20, 15, density=0.3, format="csr", dtype=np.float32, random_state=np.random.RandomState(4))
  X.data[:] = 1.0
  if negative:
    X.data[3] = -1.0
  return RecommendationDataset(X)


def _classes():
  from recoder_amd import nn
  return {"MatrixFactorization": lambda: nn.MatrixFactorization(8), "ShallowAutoencoder": nn.ShallowAutoencoder,
          "RandomWalkItemModel": nn.RandomWalkItemModel, "SparseLinearModel": nn.SparseLinearModel,
          "ItemNeighbourhoodModel": nn.ItemNeighbourhoodModel, "UserNeighbourhoodModel": nn.UserNeighbourhoodModel}


METHODS = {"train_als": "MatrixFactorization", "train_bpr": "MatrixFactorization", "train_svd": "MatrixFactorization",
           "train_ease": "ShallowAutoencoder", "train_rp3beta": "RandomWalkItemModel",
           "train_itemknn": "ItemNeighbourhoodModel", "train_slim": "SparseLinearModel",
           "train_userknn": "UserNeighbourhoodModel"}
CLASSES = ("MatrixFactorization", "ShallowAutoencoder", "RandomWalkItemModel", "SparseLinearModel",
           "ItemNeighbourhoodModel", "UserNeighbourhoodModel")


@pytest.mark.parametrize("method,wrong", [(m, c) for m in METHODS for c in CLASSES if c != METHODS[m]])
def test_a_model_of_another_class_is_a_value_error(monkeypatch, method, wrong):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_classes()[wrong]())
  with pytest.raises(ValueError) as e:
    getattr(rec, method)(_dataset())
  text = str(e.value)
  assert text.startswith(method + " ") and METHODS[method] in text and text.endswith(", not " + wrong)
  assert rec.optimizer is None and rec.items is None


def _untouched(rec, before):
  m = rec.model
  assert m.model_params() == before
  assert rec.optimizer is None and rec.sparse_optimizer is None and rec.items is None
  assert (m.interaction_values if hasattr(m, "interaction_values") else m.item_weights) is None


# (method, the model's class, one valid explicit override, one invalid argument)
REFUSED = [("train_ease", "ShallowAutoencoder", {}, {"reg": 0.0}),
           ("train_rp3beta", "RandomWalkItemModel", {"alpha": 0.9}, {"neighbours": 0}),
           ("train_itemknn", "ItemNeighbourhoodModel", {"shrink": 5.0}, {"neighbours": 0}),
           ("train_slim", "SparseLinearModel", {"l1_reg": 2.0}, {"neighbours": 0}),
           ("train_userknn", "UserNeighbourhoodModel", {"shrink": 3.0}, {"neighbours": 0})]


@pytest.mark.parametrize("method,cls,valid,invalid", REFUSED, ids=[r[0] for r in REFUSED])
def test_a_refused_argument_leaves_nothing_behind(monkeypatch, method, cls, valid, invalid):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_classes()[cls]())
  before = rec.model.model_params()
  with pytest.raises(ValueError, match=next(iter(invalid))):
    getattr(rec, method)(_dataset(), **valid, **invalid)
  _untouched(rec, before)


@pytest.mark.parametrize("method,cls,valid", [r[:3] for r in REFUSED[1:]], ids=[r[0] for r in REFUSED[1:]])
def test_a_refused_size_leaves_nothing_behind(monkeypatch, method, cls, valid):
  """The size-hint check: tables for 10^11 users and items are beyond one device whatever the model."""
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_classes()[cls](), num_users=10 ** 11, num_items=10 ** 11)
  before = rec.model.model_params()
  with pytest.raises(ValueError, match="100000000000"):
    getattr(rec, method)(_dataset(), **valid)
  _untouched(rec, before)


@pytest.mark.parametrize("method,cls,valid", [REFUSED[2][:3], REFUSED[3][:3]], ids=["train_itemknn", "train_slim"])
def test_a_refused_stored_value_leaves_nothing_behind(monkeypatch, method, cls, valid):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_classes()[cls]())
  before = rec.model.model_params()
  assert all(before[k] != v for k, v in valid.items())
  with pytest.raises(ValueError, match="1 of the 90 stored values"):
    getattr(rec, method)(_dataset(negative=True), **valid)
  _untouched(rec, before)


TRAIN_REFUSALS = {
    "ShallowAutoencoder": "a ShallowAutoencoder is fitted in closed form: call train_ease(train_dataset) "
                          "(gradient steps would not keep its zero diagonal)",
    "RandomWalkItemModel": "a RandomWalkItemModel is fitted in closed form from the interaction graph: call "
                           "train_rp3beta(train_dataset)",
    "SparseLinearModel": "a SparseLinearModel is fitted by coordinate descent on the Gram matrix: call "
                         "train_slim(train_dataset)",
    "ItemNeighbourhoodModel": "an ItemNeighbourhoodModel is fitted in closed form from the items' co-occurrences: call "
                              "train_itemknn(train_dataset)",
    "UserNeighbourhoodModel": "a UserNeighbourhoodModel is its training matrix, there is nothing to descend on: call "
                              "train_userknn(train_dataset)",
}


@pytest.mark.parametrize("cls", sorted(TRAIN_REFUSALS))
def test_train_points_at_the_closed_form_method(monkeypatch, cls):
  from recoder_amd.model import Recoder
  _no_gpu(monkeypatch)
  rec = Recoder(model=_classes()[cls]())
  with pytest.raises(ValueError) as e:
    rec.train(_dataset())
  method = [m for m, c in METHODS.items() if c == cls][0]
  assert method + "(train_dataset)" in str(e.value)
  assert str(e.value) == TRAIN_REFUSALS[cls]
  assert rec.optimizer is None and rec.items is None


def _fill(model):
  """n = 5, K = 2: two full lists, a short one with a -1 pad (and a weight under the pad that must not show),
  an empty one."""
  model.init_model(num_items=5)
  model.item_neighbours.copy_(torch.tensor([[1, 3], [0, -1], [-1, -1], [0, 4], [2, 3]], dtype=torch.int32))
  model.item_weights.data.copy_(torch.tensor([[0.5, 0.25], [1.5, 9.0], [7.0, 7.0], [2.0, 3.0], [4.0, 5.0]]))
  model.neighbour_counts.copy_(torch.tensor([2, 1, 0, 2, 2], dtype=torch.int32))
  return model


def test_dense_weights_orientation():
  from recoder_amd.nn import RandomWalkItemModel, SparseLinearModel
  by_rows = torch.tensor([[0.0, 0.5, 0.0, 0.25, 0.0],
                          [1.5, 0.0, 0.0, 0.0, 0.0],
                          [0.0, 0.0, 0.0, 0.0, 0.0],
                          [2.0, 0.0, 0.0, 0.0, 3.0],
                          [0.0, 0.0, 4.0, 5.0, 0.0]])
  by_columns = torch.tensor([[0.0, 1.5, 0.0, 2.0, 0.0],
                             [0.5, 0.0, 0.0, 0.0, 0.0],
                             [0.0, 0.0, 0.0, 0.0, 4.0],
                             [0.25, 0.0, 0.0, 0.0, 5.0],
                             [0.0, 0.0, 0.0, 3.0, 0.0]])
  rows = _fill(RandomWalkItemModel(neighbours=2))
  cols = _fill(SparseLinearModel(neighbours=2))
  assert torch.equal(rows.dense_weights(), by_rows)
  assert torch.equal(cols.dense_weights(), by_columns)
  assert rows.dense_weights(torch.float64).dtype == torch.float64
  # (the dense-input forward on the host is the product with that matrix)
  x = torch.tensor([[1.0, 0.0, 2.0, 0.0, 1.0]])
  assert torch.equal(rows(x), x @ by_rows) and torch.equal(cols(x), x @ by_columns)
