"""recoder_amd -- MI355X-native hot path of amoussawi/recoder (reference v0.4.0).

Drop-in for the reference's training path: ``Recoder`` / ``FactorizationModel``
/ losses / sparse-batch data classes keep their API; underneath, a thin C ABI
(include/recoder_hip.h, recoder_amd/csrc) of hand-written gfx950 HIP kernels.
"""
# value of the reference's recoder.__version__ (recoder/__init__.py:1); stored
# in checkpoints as 'recoder_version' (model.py:207)
__version__ = "0.4.0"

__all__ = ["ShallowAutoencoder", "RandomWalkItemModel", "SparseLinearModel", "UserNeighbourhoodModel",
           "ItemNeighbourhoodModel", "GraphFilterModel", "AdmmSlimModel", "LowRankShallowAutoencoder",
           "NeuralMatrixFactorization"]


def __getattr__(name):
  # (lazy: importing the package alone does not import torch)
  if name == "ShallowAutoencoder":
    from .nn import ShallowAutoencoder
    return ShallowAutoencoder
  if name == "RandomWalkItemModel":
    from .nn import RandomWalkItemModel
    return RandomWalkItemModel
  if name == "SparseLinearModel":
    from .nn import SparseLinearModel
    return SparseLinearModel
  if name == "UserNeighbourhoodModel":
    from .nn import UserNeighbourhoodModel
    return UserNeighbourhoodModel
  if name == "ItemNeighbourhoodModel":
    from .nn import ItemNeighbourhoodModel
    return ItemNeighbourhoodModel
  if name == "GraphFilterModel":
    from .nn import GraphFilterModel
    return GraphFilterModel
  if name == "AdmmSlimModel":
    from .nn import AdmmSlimModel
    return AdmmSlimModel
  if name == "LowRankShallowAutoencoder":
    from .nn import LowRankShallowAutoencoder
    return LowRankShallowAutoencoder
  if name == "NeuralMatrixFactorization":
    from .nn import NeuralMatrixFactorization
    return NeuralMatrixFactorization
  raise AttributeError("module %r has no attribute %r" % (__name__, name))
