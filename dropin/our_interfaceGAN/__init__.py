"""Drop-in for the reference's `our_interfaceGAN` package (a namespace package there, like `utils`): `train_boundary` and
`linear_interpolation` resolve here (MI355X path), every other module of the reference's directory keeps resolving to its own file."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
