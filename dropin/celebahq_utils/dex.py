"""our_interfaceGAN/celebahq_utils/dex/__init__.py of the reference: `eval(classifier_name)` and `estimate_score(classifier, imgs,
no_soft=False)` on transeditor_amd.celeba_attr.CelebAAttributeScorer.  The editing scripts (edit_all_noinversion_celebahq.py:175-182,
editing_evaluate.py) hand over the image already flipped to BGR and scaled to [0, 255], so the scorer takes it as it is
(preprocessed=True).  The weights are $TE_CELEBA_ATTR_DIR/<classifier_name>/net_best.pth, the reference's pth_celeba layout and its own
files; an attribute is the name of its directory."""
import os

from transeditor_amd.celeba_attr import CelebAAttributeScorer

_scorers = {}


def weights_path(classifier_name):
    d = os.environ.get('TE_CELEBA_ATTR_DIR')
    if not d:
        raise RuntimeError('celebahq_utils.dex: set TE_CELEBA_ATTR_DIR to the directory that holds <attribute>/net_best.pth '
                           "(the reference's pth_celeba)")
    path = os.path.join(d, str(classifier_name), 'net_best.pth')
    if not os.path.isfile(path):
        raise RuntimeError(f'celebahq_utils.dex: {path} not found (TE_CELEBA_ATTR_DIR={d})')
    return path


def eval(classifier_name):                                                      # noqa: A001 (the reference's name)
    """api.py:20-22: the classifier of one attribute (kept: a second call returns the same scorer)"""
    if classifier_name not in _scorers:
        _scorers[classifier_name] = CelebAAttributeScorer(weights_path(classifier_name), name=str(classifier_name))
    return _scorers[classifier_name]


def estimate_score(classifier, imgs, no_soft=False):
    """api.py:24-26: [B,3,S,S] BGR in [0, 255] on the GPU -> [B]: softmax([l, -l])[:, 1], or the logit with no_soft=True"""
    return classifier(imgs, preprocessed=True, no_soft=no_soft)
