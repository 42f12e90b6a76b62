"""The DEX age / gender scorer of attribute editing on the gfx950 kernels (the reference's our_interfaceGAN/ffhq_utils/dex/models.py:27-69
and api.py:42-65, as edit_all_noinversion_ffhq.py:113-131 calls them): a VGG16 whose last layer has 101 age or 2 gender classes.

    scorer = DEXScorer('age_sd.pth', attribute='age')               # the reference's own weight file
    s = scorer(images)                                              # [B,3,S,S] RGB in [-1, 1] -> [B]: the expected age
    p = scorer.probabilities(images)                                # [B,C]
    res = fit_boundaries(G, scorer, n_sample=10000, batch=16)       # an instance is a score_fn of transeditor_amd.edit

    python -m transeditor_amd.dex --ckpt G.pt --weights age_sd.pth --attribute age --num_sample 10000
                                  --write_z_boundary zb.npy --write_p_boundary pb.npy [--write_scores s.npy]

Weights come from a local file in the reference's key layout (conv.{0..4}.conv{1,2,3}.*, fc1.0.*, fc2.0.*, cls.*); nothing is
downloaded and torchvision is not imported.  The geometry is read from the shapes: fc1 has 512 * pool^2 inputs, the centre crop is
32 * pool pixels (224 for the real files), the hidden widths are fc1's and fc2's, the classes cls's.

Layers: te_dex_stem_fwd_f32 (RGB -> BGR, clamp / +1 / /2 / *255 / round, the centre crop, conv1_1 + ReLU in one pass), conv1_2 ...
conv5_3 on the project's 3x3 convolution with the max-pools of csrc/lpips.hip between them (the trunk PerceptualLoss and VGG16Features
run), pool5, fc1 and fc2 as te_fc_stream_f32 with bias and ReLU, then te_cls_score_f32: cls, the softmax and the score (the expected
age sum_c (c + 1) p_c, whose weights start at 1 as the reference's do, or the first class's probability) in one launch per batch.
Eval only: the two Dropout layers are the identity and there is no backward pass.

Differences from the reference, both deliberate:
  - estimate_age crops with offset:-offset (api.py:50-52), which is empty for a 224 px image and one pixel too large for an odd
    difference; here the crop is centred, any S >= crop with an even S - crop is taken and an odd difference is refused;
  - the preprocessing is part of the scorer: it takes the generator's image as it is.  preprocessed=True takes what the reference
    hands its own functions (BGR in [0, 255]) and only crops.
There is no speed bar for this path; measured, the convolution trunk is nearly all of its cost (profiles/README.md, 'DEX scorer').
"""
import math
import sys
import warnings

import torch

from . import _lib
from .edit import fit_boundaries, scorer_main, scorer_parser  # noqa: F401  (fit_boundaries: importable from here)
from .frozen_net import VGGTrunk, check_images, no_gpu, resolve, weight_bias
from .lpips import VGG_CHANNELS

BLOCK_CONVS = (2, 2, 3, 3, 3)                                         # models.py:30-36: vgg_block(..., more) per block
ATTRIBUTES = {'age': (_lib.CLS_EXPECTATION, 101), 'gender': (_lib.CLS_FIRST, 2)}     # attribute -> (score mode, the real file's classes)
_NO_GPU = no_gpu('DEXScorer')


def dex_conv_keys():
    """the 13 key prefixes conv.{block}.conv{j} in network order"""
    return [f'conv.{blk}.conv{j}' for blk, n in enumerate(BLOCK_CONVS) for j in range(1, n + 1)]


def _pair(sd, key, path, shape=(None, None)):
    return weight_bias(sd, f'{key}.weight', f'{key}.bias', shape, 'DEXScorer', path,
                       'not a DEX state dict: conv.N.convM.*, fc1.0.*, fc2.0.*, cls.*', want=None if shape[0] else '[J,K] / [J]')


def parse_state_dict(sd, path='state_dict'):
    """-> dict(convs [(w, b)] * 13, fc1 (w, b), fc2, cls, pool, crop, hidden (h1, h2), classes); ValueError naming the key that is
    missing or has the wrong shape"""
    convs, ci = [], 3
    for key, co in zip(dex_conv_keys(), VGG_CHANNELS):
        convs.append(_pair(sd, key, path, (co, ci, 3, 3)))
        ci = co
    for key in ('fc1.0', 'fc2.0', 'cls'):
        if f'{key}.weight' in sd and sd[f'{key}.weight'].ndim != 2:
            raise ValueError(f'DEXScorer: {key}.weight is {tuple(sd[f"{key}.weight"].shape)}, expected [J,K]')
    fc1, fc2, cls = _pair(sd, 'fc1.0', path), _pair(sd, 'fc2.0', path), _pair(sd, 'cls', path)
    k1 = fc1[0].shape[1]
    pool = math.isqrt(k1 // 512)
    if pool < 1 or 512 * pool * pool != k1:
        raise ValueError(f'DEXScorer: fc1.0.weight is {tuple(fc1[0].shape)}, expected [J, 512 * pool^2] (pool5 flattened)')
    if fc2[0].shape[1] != fc1[0].shape[0]:
        raise ValueError(f'DEXScorer: fc2.0.weight is {tuple(fc2[0].shape)}, expected [J, {fc1[0].shape[0]}] (fc1 has {fc1[0].shape[0]} outputs)')
    if cls[0].shape[1] != fc2[0].shape[0]:
        raise ValueError(f'DEXScorer: cls.weight is {tuple(cls[0].shape)}, expected [C, {fc2[0].shape[0]}] (fc2 has {fc2[0].shape[0]} outputs)')
    if not 1 <= cls[0].shape[0] <= 1024:
        raise ValueError(f'DEXScorer: cls.weight is {tuple(cls[0].shape)}, expected 1 to 1024 classes')
    return dict(convs=convs, fc1=fc1, fc2=fc2, cls=cls, pool=pool, crop=32 * pool, hidden=(fc1[0].shape[0], fc2[0].shape[0]),
                classes=cls[0].shape[0])


class DEXScorer(VGGTrunk, torch.nn.Module):
    def __init__(self, path=None, state_dict=None, attribute='age'):
        super().__init__()
        if attribute not in ATTRIBUTES:
            raise ValueError(f"DEXScorer: attribute must be 'age' or 'gender', got {attribute!r}")
        state_dict, path = resolve(path, state_dict, 'DEXScorer', f'DEX {attribute}')
        net = parse_state_dict(state_dict, path)
        self.attribute, (self.mode, real) = attribute, ATTRIBUTES[attribute]
        self.pool, self.crop, self.hidden, self.classes = net['pool'], net['crop'], net['hidden'], net['classes']
        if self.classes != real:
            warnings.warn(f"DEXScorer: attribute '{attribute}' with {self.classes} classes (the reference's {attribute} file has {real})",
                          RuntimeWarning, stacklevel=2)
        self._freeze(net['convs'], [(f'{name}_{t}', v) for name in ('fc1', 'fc2', 'cls') for t, v in zip('wb', net[name])])

    def _features(self, images, preprocessed):
        """[B,3,S,S] -> fc2's output [B,hidden[1]]; an activation is dropped once the next layer has read it"""
        check_images(images, 'DEXScorer', '[B,3,S,S]', square=True)
        S = images.shape[2]
        if S < self.crop or (S - self.crop) % 2:
            raise ValueError(f'DEXScorer: the {self.crop} px centre crop needs S >= {self.crop} with S - {self.crop} even, got {S}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        x = images.detach().float()
        o = (S - self.crop) // 2

        def stem():
            if preprocessed:
                return _lib.vgg_stem_fwd(x[:, :, o:o + self.crop, o:o + self.crop].contiguous(), self._w(0), self.b0)
            return _lib.dex_stem_fwd(x, self._w(0), self.b0, self.crop)
        a = self._walk(stem)
        a = _lib.maxpool2_fwd(a).view(a.shape[0], -1)                          # pool5 + x.view(in_size, -1)
        a = _lib.fc_stream(a, self.fc1_w, self.fc1_b, act=1)                   # fc1 (Dropout: identity)
        return _lib.fc_stream(a, self.fc2_w, self.fc2_b, act=1)                # fc2

    @torch.no_grad()
    def forward(self, images, preprocessed=False):
        """[B,3,S,S] RGB in [-1, 1] (preprocessed=True: BGR in [0, 255]) -> [B] fp32 on the device: the expected age or p_0"""
        return _lib.cls_score(self._features(images, preprocessed), self.cls_w, self.cls_b, self.mode)

    @torch.no_grad()
    def probabilities(self, images, preprocessed=False):
        """-> [B,C] fp32 on the device: the softmax over the classes"""
        return _lib.cls_score(self._features(images, preprocessed), self.cls_w, self.cls_b, self.mode, want_prob=True)[1]


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = scorer_parser('score sampled images with the DEX age / gender classifier and fit the z+ and p+ editing boundaries '
                           '(edit_all_noinversion_ffhq.py:103-166)',
                           "the DEX state dict in the reference's layout (age_sd.pth / gender_sd.pth)")
    parser.add_argument('--attribute', choices=sorted(ATTRIBUTES), default='age')
    return parser


def main(argv=None):
    def make_scorer(args):
        scorer = DEXScorer(args.weights, attribute=args.attribute)
        return scorer, {'attribute': args.attribute}, {'classes': scorer.classes, 'crop': scorer.crop}
    return scorer_main(build_parser(), argv, _NO_GPU, make_scorer)


if __name__ == '__main__':
    main(sys.argv[1:])
