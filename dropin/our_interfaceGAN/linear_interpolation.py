"""our_interfaceGAN/linear_interpolation.py:4-48 of the reference (numpy in, numpy out; torch tensors are taken too)."""
from transeditor_amd.edit import linear_interpolate                                                 # noqa: F401
