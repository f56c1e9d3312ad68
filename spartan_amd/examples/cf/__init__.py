"""Collaborative filtering (the reference's spartan/examples/cf package): `ItemBasedRecommender`."""
from .item_recommender import ItemBasedRecommender  # noqa: F401
