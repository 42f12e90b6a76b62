"""our_interfaceGAN/ffhq_utils/dex/__init__.py of the reference: `eval(attribute_name)`, `estimate_age(img)` and `estimate_gender(img)` on
transeditor_amd.dex.DEXScorer.  The editing scripts (edit_all_noinversion_ffhq.py:113-121) hand over the image already flipped to BGR
and scaled to [0, 255], so the scorer only crops (preprocessed=True).  The weights are $TE_DEX_DIR/age_sd.pth and
$TE_DEX_DIR/gender_sd.pth, the reference's own files.  Only the two DEX attributes exist here (the CelebA-HQ attribute classifiers are
dropin/celebahq_utils/dex.py; there is no pose classifier); the centre crop takes any size with an even margin, a 224 px image included
(api.py:50-52 returns an empty crop for it)."""
import os

from transeditor_amd.dex import DEXScorer

FILES = {'age': 'age_sd.pth', 'gender': 'gender_sd.pth'}
_scorers = {}


def weights_path(attribute):
    d = os.environ.get('TE_DEX_DIR')
    if not d:
        raise RuntimeError(f'ffhq_utils.dex: set TE_DEX_DIR to the directory that holds {FILES["age"]} and {FILES["gender"]}')
    path = os.path.join(d, FILES[attribute])
    if not os.path.isfile(path):
        raise RuntimeError(f'ffhq_utils.dex: {path} not found (TE_DEX_DIR={d})')
    return path


def _scorer(attribute):
    if attribute not in _scorers:
        _scorers[attribute] = DEXScorer(weights_path(attribute), attribute=attribute)
    return _scorers[attribute]


def eval(attribute_name):                                                       # noqa: A001 (the reference's name)
    """api.py:21-39: load the classifier behind estimate_age / estimate_gender"""
    if attribute_name not in FILES:
        raise ValueError(f"ffhq_utils.dex.eval: only 'age' and 'gender' exist here, got {attribute_name!r}")
    _scorer(attribute_name)


def estimate_age(img):
    """[B,3,S,S] BGR in [0, 255] on the GPU -> [B]: sum_c (c + 1) p_c"""
    return _scorer('age')(img, preprocessed=True)


def estimate_gender(img):
    """[B,3,S,S] BGR in [0, 255] on the GPU -> [B]: the first class's probability"""
    return _scorer('gender')(img, preprocessed=True)
