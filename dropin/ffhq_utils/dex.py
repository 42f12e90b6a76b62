"""our_interfaceGAN/ffhq_utils/dex/__init__.py of the reference: `eval(attribute_name)`, `estimate_age(img)` and `estimate_gender(img)` on
transeditor_amd.dex.DEXScorer, and `estimate_pose(img)` on transeditor_amd.pose.PoseScorer.  The editing scripts
(edit_all_noinversion_ffhq.py:113-121) hand over the image already flipped to BGR and scaled to [0, 255], so the scorers only crop
(preprocessed=True).  The weights are $TE_DEX_DIR/age_sd.pth, $TE_DEX_DIR/gender_sd.pth and $TE_DEX_DIR/classifier/pose/weight.pkl, the
reference's own files under its pth/ directory.  The reference scores pose by eval('pose') followed by estimate_gender (api.py:34-39
swaps the model behind that function); here eval() knows the two DEX attributes only and pose has a function of its own,
estimate_pose (the CelebA-HQ attribute classifiers are dropin/celebahq_utils/dex.py).  The centre crop takes any size with an even
margin, a 224 px image included (api.py:50-52 returns an empty crop for it)."""
import os

from transeditor_amd.dex import DEXScorer
from transeditor_amd.pose import PoseScorer

FILES = {'age': 'age_sd.pth', 'gender': 'gender_sd.pth'}
POSE_FILE = os.path.join('classifier', 'pose', 'weight.pkl')
_scorers = {}


def weights_path(attribute):
    name = POSE_FILE if attribute == 'pose' else FILES[attribute]
    d = os.environ.get('TE_DEX_DIR')
    if not d:
        raise RuntimeError(f'ffhq_utils.dex: set TE_DEX_DIR to the directory that holds {FILES["age"]} and {FILES["gender"]}'
                           + (f' (and {POSE_FILE})' if attribute == 'pose' else ''))
    path = os.path.join(d, name)
    if not os.path.isfile(path):
        raise RuntimeError(f'ffhq_utils.dex: {path} not found (TE_DEX_DIR={d})')
    return path


def _scorer(attribute):
    if attribute not in _scorers:
        path = weights_path(attribute)
        _scorers[attribute] = PoseScorer(path) if attribute == 'pose' else DEXScorer(path, attribute=attribute)
    return _scorers[attribute]


def eval(attribute_name):                                                       # noqa: A001 (the reference's name)
    """api.py:21-39: load the classifier behind estimate_age / estimate_gender"""
    if attribute_name not in FILES:
        raise ValueError(f"ffhq_utils.dex.eval: only 'age' and 'gender' exist here, got {attribute_name!r}"
                         + (' (pose is estimate_pose / transeditor_amd.pose.PoseScorer)' if attribute_name == 'pose' else ''))
    _scorer(attribute_name)


def estimate_age(img):
    """[B,3,S,S] BGR in [0, 255] on the GPU -> [B]: sum_c (c + 1) p_c"""
    return _scorer('age')(img, preprocessed=True)


def estimate_gender(img):
    """[B,3,S,S] BGR in [0, 255] on the GPU -> [B]: the first class's probability"""
    return _scorer('gender')(img, preprocessed=True)


def estimate_pose(img):
    """[B,3,S,S] BGR in [0, 255] on the GPU -> [B]: the first class's probability of the ResNet-18 pose classifier"""
    return _scorer('pose')(img, preprocessed=True)
