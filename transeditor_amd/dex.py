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
import argparse
import json
import math
import sys
import warnings

import numpy as np
import torch

from . import _lib
from .lpips import POOL_AFTER, VGG_CHANNELS, VGGTrunk, _load

BLOCK_CONVS = (2, 2, 3, 3, 3)                                         # models.py:30-36: vgg_block(..., more) per block
ATTRIBUTES = {'age': (_lib.CLS_EXPECTATION, 101), 'gender': (_lib.CLS_FIRST, 2)}     # attribute -> (score mode, the real file's classes)
_NO_GPU = 'DEXScorer needs a GPU (the network runs on the gfx950 kernels only; there is no CPU path)'


def dex_conv_keys():
    """the 13 key prefixes conv.{block}.conv{j} in network order"""
    return [f'conv.{blk}.conv{j}' for blk, n in enumerate(BLOCK_CONVS) for j in range(1, n + 1)]


def _pair(sd, key, path, shape=None):
    kw, kb = f'{key}.weight', f'{key}.bias'
    if kw not in sd or kb not in sd:
        raise ValueError(f'DEXScorer: {path} has no {kw} / {kb} (not a DEX state dict: conv.N.convM.*, fc1.0.*, fc2.0.*, cls.*)')
    w, b = sd[kw], sd[kb]
    if shape is not None and tuple(w.shape) != shape or b.ndim != 1 or b.shape[0] != w.shape[0]:
        want = f'{shape} / {(shape[0],)}' if shape is not None else '[J,K] / [J]'
        raise ValueError(f'DEXScorer: {kw} is {tuple(w.shape)} / bias {tuple(b.shape)}, expected {want}')
    return w.detach().float().contiguous(), b.detach().float().contiguous()


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
        if state_dict is None:
            state_dict = _load(path, f'DEX {attribute}', who='DEXScorer')
        else:
            if path is not None:
                raise ValueError('DEXScorer: give path or state_dict, not both')
            if not isinstance(state_dict, dict):
                raise ValueError(f'DEXScorer: state_dict must be a dict, got {type(state_dict).__name__}')
            path = 'state_dict'
        net = parse_state_dict(state_dict, path)
        self.attribute, (self.mode, real) = attribute, ATTRIBUTES[attribute]
        self.pool, self.crop, self.hidden, self.classes = net['pool'], net['crop'], net['hidden'], net['classes']
        if self.classes != real:
            warnings.warn(f"DEXScorer: attribute '{attribute}' with {self.classes} classes (the reference's {attribute} file has {real})",
                          RuntimeWarning, stacklevel=2)
        for i, (w, b) in enumerate(net['convs']):
            self.register_buffer(f'w{i}', w)
            self.register_buffer(f'b{i}', b)
        for name in ('fc1', 'fc2', 'cls'):
            self.register_buffer(f'{name}_w', net[name][0])
            self.register_buffer(f'{name}_b', net[name][1])
        self._packs = {}
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _features(self, images, preprocessed):
        """[B,3,S,S] -> fc2's output [B,hidden[1]]; an activation is dropped once the next layer has read it"""
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError(f'DEXScorer: expected [B,3,S,S] images, got {tuple(images.shape)}')
        S = images.shape[2]
        if images.shape[3] != S:
            raise ValueError(f'DEXScorer: the images must be square, got {images.shape[2]}x{images.shape[3]}')
        if S < self.crop or (S - self.crop) % 2:
            raise ValueError(f'DEXScorer: the {self.crop} px centre crop needs S >= {self.crop} with S - {self.crop} even, got {S}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        x = images.detach().float()
        if preprocessed:
            o = (S - self.crop) // 2
            a = _lib.vgg_stem_fwd(x[:, :, o:o + self.crop, o:o + self.crop].contiguous(), self._w(0), self.b0)
        else:
            a = _lib.dex_stem_fwd(x, self._w(0), self.b0, self.crop)
        for i in range(1, 13):
            if (i - 1) in POOL_AFTER:
                a = _lib.maxpool2_fwd(a)
            a = self._conv_fwd(i, a)
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


def fit_boundaries(generator, scorer, *, n_sample, batch, ratio=0.02, split_ratio=0.7, truncation=0.7, seed=None, latent=512,
                   para_num=16, invalid_value=None):
    """edit_all_noinversion_ffhq.py:103-166: sample n_sample codes, score their images with `scorer` and fit one boundary in z+ and one
    in p+ to the extreme scores (edit.sample_codes, then edit.train_boundary twice; `seed` seeds the sampling and both splits).
    -> dict(z_boundary, p_boundary: [1, tokens * latent] float32 numpy, unit norm; z_report, p_report: train_boundary's reports;
            scores: [n_sample, 1] on the device)"""
    from . import edit
    z_codes, p_codes, scores = edit.sample_codes(generator, scorer, n_sample=n_sample, batch=batch, truncation=truncation, seed=seed,
                                                 latent=latent, para_num=para_num)
    z_boundary, z_report = edit.train_boundary(z_codes, scores, ratio, split_ratio, invalid_value, seed)
    p_boundary, p_report = edit.train_boundary(p_codes, scores, ratio, split_ratio, invalid_value, seed)
    return dict(z_boundary=z_boundary, p_boundary=p_boundary, z_report=z_report, p_report=p_report, scores=scores)


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = argparse.ArgumentParser(description='score sampled images with the DEX age / gender classifier and fit the z+ and p+ editing '
                                                 'boundaries (edit_all_noinversion_ffhq.py:103-166)')
    parser.add_argument('--ckpt', required=True, help='a generator checkpoint file')
    parser.add_argument('--weights', required=True, help="the DEX state dict in the reference's layout (age_sd.pth / gender_sd.pth)")
    parser.add_argument('--attribute', choices=sorted(ATTRIBUTES), default='age')
    parser.add_argument('--num_sample', type=int, default=10000)
    parser.add_argument('--write_z_boundary', required=True, help='output .npy file of the z+ boundary [1,D]')
    parser.add_argument('--write_p_boundary', required=True, help='output .npy file of the p+ boundary [1,D]')
    parser.add_argument('--write_scores', help='output .npy file of the scores [N,1]')
    parser.add_argument('--ratio', type=float, default=0.02, help='chosen_num_or_ratio')
    parser.add_argument('--split_ratio', type=float, default=0.7)
    parser.add_argument('--seed', type=int, default=None, help='seed of the sampled codes and of the train / validation splits')
    parser.add_argument('--size', type=int, default=256)
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--truncation', type=float, default=0.7)
    parser.add_argument('--para_num', type=int, default=16)
    parser.add_argument('--channel_multiplier', type=int, default=2)
    parser.add_argument('--num_trans', type=int, default=8)
    return parser


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.size < 8 or args.size & (args.size - 1):
        parser.error(f'--size must be a power of two >= 8, got {args.size}')
    if args.num_sample < 1 or args.batch < 1:
        parser.error('--num_sample and --batch must be positive')
    if not torch.cuda.is_available():
        raise RuntimeError(_NO_GPU)
    from .inference import GeneratorSampler
    from .model_spatial_query import Generator
    from .train_step import load_checkpoint_into
    scorer = DEXScorer(args.weights, attribute=args.attribute)
    g = Generator(args.size, 512, 512, 2 * (int(math.log(args.size, 2)) - 1), channel_multiplier=args.channel_multiplier,
                  n_trans=args.num_trans, pixel_norm_op_dim=1).to('cuda')
    load_checkpoint_into(args.ckpt, g, device='cuda', g_ema_only_ok=True)
    out = fit_boundaries(GeneratorSampler(g), scorer, n_sample=args.num_sample, batch=args.batch, ratio=args.ratio,
                         split_ratio=args.split_ratio, truncation=args.truncation, seed=args.seed, para_num=args.para_num)
    np.save(args.write_z_boundary, out['z_boundary'])
    np.save(args.write_p_boundary, out['p_boundary'])
    scores = out['scores'].cpu().numpy()
    if args.write_scores:
        np.save(args.write_scores, scores)
    res = {'attribute': args.attribute, 'ckpt': args.ckpt, 'weights': args.weights, 'n': args.num_sample, 'classes': scorer.classes,
           'crop': scorer.crop, 'score_mean': float(scores.mean()), 'score_min': float(scores.min()), 'score_max': float(scores.max()),
           'z': out['z_report'], 'p': out['p_report'], 'wrote': [args.write_z_boundary, args.write_p_boundary] +
           ([args.write_scores] if args.write_scores else [])}
    print(json.dumps(res), flush=True)
    return res


if __name__ == '__main__':
    main(sys.argv[1:])
