"""our_interfaceGAN/train_boundary.py:5-139 of the reference: numpy codes and scores in, the [1,D] unit boundary out."""
from transeditor_amd.edit import reference_train_boundary as train_boundary                         # noqa: F401
