"""Drop-in for the reference's `metrics` package (a namespace package there, like `utils`): `metrics.inception` resolves here (MI355X
path, no torchvision, no download), every other module of the reference's directory keeps resolving to its own file."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
