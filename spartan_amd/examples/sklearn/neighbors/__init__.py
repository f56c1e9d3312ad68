"""Nearest-neighbour search (interface of the reference's spartan/examples/sklearn/neighbors): `NearestNeighbors`."""
from .unsupervised import NearestNeighbors  # noqa: F401
