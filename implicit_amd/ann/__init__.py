"""Approximate-nearest-neighbour wrappers around a fitted matrix-factorisation model (the reference's implicit/ann).  One
index exists here, a native IVF-Flat one (implicit_amd.gpu.IVFIndex); annoy and nmslib have no counterpart."""
from .ivf import IVFModel

__all__ = ["IVFModel"]
