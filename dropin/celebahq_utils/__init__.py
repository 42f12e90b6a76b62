"""Drop-in for the reference's `our_interfaceGAN/celebahq_utils` package (a namespace package there): `celebahq_utils.dex` resolves here
(MI355X path), anything else of the reference's directory keeps resolving to its own file."""
from pkgutil import extend_path

__path__ = extend_path(__path__, __name__)
