"""Manifold learning (interface of the reference's spartan/examples/sklearn/manifold): `Isomap`."""
from .isomap import Isomap  # noqa: F401
