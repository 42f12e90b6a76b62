"""The CelebA-HQ attribute classifiers of attribute editing on the gfx950 kernels (the reference's our_interfaceGAN/celebahq_utils/dex/
networks/classifiers/attribute_classifier.py:152-215, D with fixed_size=True and use_mbstd=False, wrapped by attribute_utils.py:8-60, as
edit_all_noinversion_celebahq.py:136, :175-182 and editing_evaluate.py call them): a progressive-GAN discriminator with one logit.

    scorer = CelebAAttributeScorer('pth_celeba/Smiling/net_best.pth')   # the reference's own weight file
    s = scorer(images)                                                  # [B,3,S,S] RGB in [-1, 1] -> [B]: softmax([l, -l])[:, 1]
    l = scorer.logits(images)                                           # [B]: the logit
    scorers = load_scorers('pth_celeba', ['Smiling', 'Male'])           # {name: scorer}, for edit_eval.score_sweeps
    res = edit.fit_boundaries(G, scorer, n_sample=10000, batch=16)      # an instance is a score_fn of transeditor_amd.edit

    python -m transeditor_amd.celeba_attr --ckpt G.pt --weights net_best.pth [--name Smiling] --num_sample 10000
                                          --write_z_boundary zb.npy --write_p_boundary pb.npy [--write_scores s.npy] [--no_soft]

Weights come from a local file in the reference's layout ({'state_dict': ..., 'epoch', 'valacc'}; keys fromrgb_lod0.conv.*,
{r}x{r}.conv{0,1}.*, 4x4.conv.*, 4x4.dense{0,1}.*); nothing is downloaded.  The geometry is read from the shapes: the resolution R is the
largest {r}x{r} block (256 for the real files), the channel counts are the weights'.  The constant scales of the equalised learning rate
(gain / sqrt(fan-in), gain sqrt(2), for dense1 1) are multiplied into the weights once, at load time.

Layers: te_attr_stem_fwd_f32 (RGB -> BGR, clamp / +1 / /2 / *255 / round, the S / R box mean, fromrgb_lod0 + leaky ReLU in one pass);
per block conv0 on the project's 3x3 convolution with bias and leaky ReLU in its epilogue, conv1 with bias only, then
te_avgpool2_act_f32 (the reference's order: conv -> bias -> downscale -> act); the 4x4 convolution; dense0 as te_fc_stream_f32; then
te_attr_score_f32: dense0's activation, dense1 and the score in one launch per batch.  Eval only, no backward pass.

Two quirks of the reference are kept: the network sees BGR byte levels (the editing scripts flip and scale the image before they call
it), and the score is softmax([l, -l])[:, 1] = 1 / (1 + exp(2 l)), which DECREASES in the logit.  The preprocessing is part of the
scorer, which takes the generator's image as it is; preprocessed=True takes what the reference hands its own classifier.  An image
larger than R is box-averaged down (attribute_utils.downsample, for any R), a smaller one is refused.
There is no speed bar for this path; see profiles/README.md, 'CelebA-HQ attribute scorer'.
"""
import math
import os
import re
import sys

import torch

from . import _lib
from .edit import scorer_main, scorer_parser
from .frozen_net import FrozenConvs, check_images, no_gpu, resolve, weight_bias
from .op import modconv

SLOPE = 0.2
_NO_GPU = no_gpu('CelebAAttributeScorer')
_LAYOUT = 'not an attribute classifier state dict: fromrgb_lod0.conv.*, {r}x{r}.conv{0,1}.*, 4x4.conv.*, 4x4.dense{0,1}.*'
_BLOCK = re.compile(r'^(\d+)x\1\.conv0\.conv\.weight$')


def _pair(sd, prefix, kind, path, shape):
    """(weight, bias) of one layer; `shape` is the expected weight shape with None where the state dict decides"""
    return weight_bias(sd, f'{prefix}.{kind}.weight', f'{prefix}.wscale.b', shape, 'CelebAAttributeScorer', path, _LAYOUT,
                       want='(' + ', '.join('*' if s is None else str(s) for s in shape) + ') / (Co,)')


def _scaled(w, gain2):
    """w * gain / sqrt(fan-in), gain2 = gain^2 (WScaleLayer's constant, folded in: conv(x, w) * s == conv(x, w * s))"""
    return (w * math.sqrt(gain2 / w[0].numel())).contiguous()


def parse_state_dict(sd, path='state_dict'):
    """-> dict(resolution, channels (the stem's, then every convolution's outputs), stem (w [C0,3], b), convs [(w, b)] in network order
    ({R}x{R}.conv0, .conv1, ..., 8x8.conv1, 4x4.conv), dense0 (w [J,C*16], b), dense1 (w [J], b [1])), every weight with its constant
    scale folded in.  Takes the bare state dict or the reference's {'state_dict': ...} file content; lod_in and fromrgb_lod{i > 0}.* are
    ignored.  ValueError naming the key that is missing or has the wrong shape."""
    if isinstance(sd.get('state_dict'), dict):
        sd = sd['state_dict']
    sizes = sorted(int(m.group(1)) for m in map(_BLOCK.match, (k for k in sd if isinstance(k, str))) if m)
    if not sizes:
        raise ValueError(f'CelebAAttributeScorer: {path} has no {{r}}x{{r}}.conv0.conv.weight ({_LAYOUT})')
    R = sizes[-1]
    if R < 8 or R & (R - 1):
        raise ValueError(f'CelebAAttributeScorer: the largest block of {path} is {R}x{R}.conv0.conv.weight, expected a power of two >= 8')
    w, b = _pair(sd, 'fromrgb_lod0.conv', 'conv', path, (None, 3, 1, 1))
    stem = (_scaled(w, 2.0).view(-1, 3).contiguous(), b)
    if w.shape[0] > 1024:
        raise ValueError(f'CelebAAttributeScorer: fromrgb_lod0.conv.conv.weight is {tuple(w.shape)}, expected at most 1024 channels')
    channels, convs, c, r = [w.shape[0]], [], w.shape[0], R
    while r >= 8:
        for j in (0, 1):
            w, b = _pair(sd, f'{r}x{r}.conv{j}', 'conv', path, (None, c, 3, 3))
            convs.append((_scaled(w, 2.0), b))
            c = w.shape[0]
            channels.append(c)
        r //= 2
    w, b = _pair(sd, '4x4.conv', 'conv', path, (None, c, 3, 3))
    convs.append((_scaled(w, 2.0), b))
    c = w.shape[0]
    channels.append(c)
    w0, b0 = _pair(sd, '4x4.dense0', 'linear', path, (None, c * 16))
    if w0.shape[0] % 4:
        raise ValueError(f'CelebAAttributeScorer: 4x4.dense0.linear.weight is {tuple(w0.shape)}, expected a multiple of 4 outputs')
    w1, b1 = _pair(sd, '4x4.dense1', 'linear', path, (1, w0.shape[0]))
    return dict(resolution=R, channels=tuple(channels), stem=stem, convs=convs, dense0=(_scaled(w0, 2.0), b0),
                dense1=(_scaled(w1, 1.0).view(-1).contiguous(), b1))


class CelebAAttributeScorer(FrozenConvs, torch.nn.Module):
    """buffers: stem_w / stem_b, w{i} / b{i} of convolution i (FrozenConvs's names), dense0_w / dense0_b,
    dense1_w / dense1_b; all weights scaled"""

    def __init__(self, path=None, state_dict=None, name=None):
        super().__init__()
        state_dict, path = resolve(path, state_dict, 'CelebAAttributeScorer', f'attribute classifier{f" {name!r}" if name else ""}')
        net = parse_state_dict(state_dict, path)
        self.name, self.resolution, self.channels = name, net['resolution'], net['channels']
        self.register_buffer('stem_w', net['stem'][0])
        self.register_buffer('stem_b', net['stem'][1])
        self.n_convs = len(net['convs'])
        self._freeze(net['convs'], [(f'{key}_{t}', v) for key in ('dense0', 'dense1') for t, v in zip('wb', net[key])])

    def train(self, mode=True):
        if mode:
            raise RuntimeError('CelebAAttributeScorer is eval only (there is no backward pass)')
        return super().train(False)

    def conv_routes(self, B):
        """[(H, convolution kind code)] of the 3x3 convolutions for a batch of B, in network order: what modconv.fwd_kinds selects"""
        out, H = [], self.resolution
        for i in range(self.n_convs):
            out.append((H, modconv.fwd_kinds('3x3', B, self._w(i), H, H)[1]))
            if i % 2 == 1:
                H //= 2
        return out

    def _dense0(self, images, preprocessed):
        """[B,3,S,S] -> dense0's output before its activation [B,J]; an activation is dropped once the next layer has read it"""
        check_images(images, 'CelebAAttributeScorer', '[B,3,S,S]', square=True)
        S, R = images.shape[2], self.resolution
        if S < R or S % R:
            raise ValueError(f'CelebAAttributeScorer: the image size must be a multiple of the resolution {R}, got {S}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        a = _lib.attr_stem_fwd(images.detach().float(), self.stem_w, self.stem_b, R, preprocessed)
        for i in range(0, self.n_convs - 1, 2):
            a = self._conv(i, a, 4)                                            # conv0 + bias + leaky ReLU
            a = self._conv(i + 1, a, 0)                                        # conv1 + bias
            a = _lib.avgpool2_act(a, SLOPE)                                    # downscale, then the activation
        a = self._conv(self.n_convs - 1, a, 4).view(a.shape[0], -1)            # the 4x4 convolution + x.view([B, -1])
        return _lib.fc_stream(a, self.dense0_w, self.dense0_b, act=0)

    @torch.no_grad()
    def forward(self, images, preprocessed=False, no_soft=False):
        """[B,3,S,S] RGB in [-1, 1] (preprocessed=True: BGR in [0, 255]), S a multiple of the resolution -> [B] fp32 on the device:
        softmax([l, -l])[:, 1], or the logit l with no_soft=True (ClassifierWrapper.forward, attribute_utils.py:55-60)"""
        logit, score = _lib.attr_score(self._dense0(images, preprocessed), self.dense1_w, self.dense1_b, SLOPE, want_logit=no_soft,
                                       want_score=not no_soft)
        return logit if no_soft else score

    def logits(self, images, preprocessed=False):
        """-> [B] fp32 on the device: the logit"""
        return self.forward(images, preprocessed=preprocessed, no_soft=True)


def load_scorers(directory, names):
    """{name: CelebAAttributeScorer(<directory>/<name>/net_best.pth)}: the reference's pth_celeba layout, an attribute being the name
    of its directory"""
    return {name: CelebAAttributeScorer(os.path.join(directory, name, 'net_best.pth'), name=name) for name in names}


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = scorer_parser('score sampled images with a CelebA-HQ attribute classifier and fit the z+ and p+ editing boundaries '
                           '(edit_all_noinversion_celebahq.py:136-240)', "the classifier's net_best.pth in the reference's layout")
    parser.add_argument('--name', default=None, help='the attribute (reported only), e.g. Smiling')
    parser.add_argument('--no_soft', action='store_true', help='score with the logit instead of softmax([l, -l])[:, 1]')
    return parser


def main(argv=None):
    def make_scorer(args):
        scorer = CelebAAttributeScorer(args.weights, name=args.name)
        score_fn = (lambda images: scorer(images, no_soft=True)) if args.no_soft else scorer
        return score_fn, {'name': args.name}, {'resolution': scorer.resolution, 'channels': list(scorer.channels),
                                               'no_soft': bool(args.no_soft)}
    return scorer_main(build_parser(), argv, _NO_GPU, make_scorer)


if __name__ == '__main__':
    main(sys.argv[1:])
