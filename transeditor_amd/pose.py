"""The pose scorer of attribute editing on the gfx950 kernels (the reference's our_interfaceGAN/ffhq_utils/dex/models.py:73-89 ClassifyModel
and api.py:34-39, :61-65, as edit_all_noinversion_ffhq.py:113-131 calls them with --attribute_name pose): torchvision's resnet18 without
its fc, Linear(512, 2) and a softmax, whose first class's probability is the score.

    scorer = PoseScorer('weight.pkl')                               # the reference's own pth/classifier/pose/weight.pkl
    s = scorer(images)                                              # [B,3,S,S] RGB in [-1, 1] -> [B]: p_0
    p = scorer.probabilities(images)                                # [B,2]
    res = fit_boundaries(G, scorer, n_sample=10000, batch=16)       # an instance is a score_fn of transeditor_amd.edit

    python -m transeditor_amd.pose --ckpt G.pt --weights weight.pkl --num_sample 10000
                                   --write_z_boundary zb.npy --write_p_boundary pb.npy [--write_scores s.npy]

Weights come from a local file with ClassifyModel's keys (backbone.0.weight, backbone.1.{weight,bias,running_mean,running_var},
backbone.{4..7}.{0,1}.{conv1,bn1,conv2,bn2}.*, backbone.{5..7}.0.downsample.{0,1}.*, extra_layer.{weight,bias}; num_batches_tracked is
ignored); nothing is downloaded and torchvision is not imported.  The geometry is read from the shapes: the four widths are the
first convolutions' of backbone.4 ... backbone.7 (64, 128, 256, 512 for the real file), the classes extra_layer's.  The centre crop is
the reference's CenterCrop(224) unless `crop` says otherwise.

Every BatchNorm2d (eps 1e-5, eval) is folded into its convolution when the weights are loaded, in fp64 on the host and rounded once
(inception_features.fold_bn).  Layers: te_pose_stem_fwd_f32 (RGB -> BGR, clamp / +1 / /2 / *255 / round, the centre crop and conv1 +
bn1 + ReLU in one pass), te_maxpool3s2p1_f32, then eight basic blocks: the first convolution (and the 1x1 stride-2 downsample of
backbone.{5,6,7}.0) on te_conv2d_f32, the second on te_conv2d_res_f32, which adds the block's input before the ReLU; the global average
is te_adaptive_avgpool_f32 and extra_layer + softmax + [:, 0] one te_cls_score_f32 launch.  Every convolution is the exact-fp32
implicit GEMM of csrc/conv2d_body.h: the planes are 56, 28, 14 and 7 pixels wide, which no split-bf16 route takes.  An image's score
is bitwise the same whatever batch it is in.  Eval only: there is no backward pass.

As in transeditor_amd.dex the preprocessing is part of the scorer (preprocessed=True takes what the reference hands its own functions,
BGR in [0, 255], and only crops), any S >= crop with an even S - crop is taken and an odd difference is refused.
Measured times and shares: profiles/README.md, 'Pose scorer'.
"""
import sys

import torch

from . import _lib
from .edit import fit_boundaries, scorer_main, scorer_parser  # noqa: F401  (fit_boundaries: importable from here)
from .frozen_net import check_images, no_gpu, resolve, weight_bias
from .inception_features import fold_bn

BN_EPS = 1e-5
CROP = 224                                                            # api.py:62
LAYERS = (4, 5, 6, 7)                                                 # resnet18's layer1 ... layer4 among the backbone's children
_NO_GPU = no_gpu('PoseScorer')
_HINT = 'not a ClassifyModel state dict: backbone.N.*, extra_layer.*'
_BN_KEYS = ('weight', 'bias', 'running_mean', 'running_var')


def pose_conv_keys():
    """[(convolution key, batch norm key, stride, padding, has a residual)] * 20 in the order forward() runs them: the stem, then
    per block conv1, the downsample where the block has one, conv2"""
    out = [('backbone.0', 'backbone.1', 2, 3, False)]
    for at, layer in enumerate(LAYERS):
        for blk in (0, 1):
            n, first = f'backbone.{layer}.{blk}', at > 0 and blk == 0
            out.append((f'{n}.conv1', f'{n}.bn1', 2 if first else 1, 1, False))
            if first:
                out.append((f'{n}.downsample.0', f'{n}.downsample.1', 2, 0, False))
            out.append((f'{n}.conv2', f'{n}.bn2', 1, 1, True))
    return out


def parse_state_dict(sd, path='state_dict'):
    """-> dict(convs {key: (w', b')} with the batch norms folded in, extra (w, b), widths (w1, w2, w3, w4), classes); ValueError
    naming the key that is missing or has the wrong shape"""
    def get(key, shape):
        return weight_bias(sd, key, None, shape, 'PoseScorer', path, _HINT)

    def conv(key, bn, co, ci, k):
        w = get(f'{key}.weight', (co, ci, k, k))
        return fold_bn(w, *(get(f'{bn}.{t}', (w.shape[0],)) for t in _BN_KEYS), eps=BN_EPS)
    convs, widths = {}, []
    convs['backbone.0'] = conv('backbone.0', 'backbone.1', None, 3, 7)
    ci = convs['backbone.0'][0].shape[0]
    for at, layer in enumerate(LAYERS):
        for blk in (0, 1):
            n, first = f'backbone.{layer}.{blk}', at > 0 and blk == 0
            convs[f'{n}.conv1'] = conv(f'{n}.conv1', f'{n}.bn1', None if first else ci, ci, 3)      # (layer1 has no downsample: its width is the stem's)
            co = convs[f'{n}.conv1'][0].shape[0]
            if first:
                convs[f'{n}.downsample.0'] = conv(f'{n}.downsample.0', f'{n}.downsample.1', co, ci, 1)
            convs[f'{n}.conv2'] = conv(f'{n}.conv2', f'{n}.bn2', co, co, 3)
            ci = co
        widths.append(ci)
    extra = weight_bias(sd, 'extra_layer.weight', 'extra_layer.bias', (None, ci), 'PoseScorer', path, _HINT)
    if not 1 <= extra[0].shape[0] <= 1024 or ci % 4:
        raise ValueError(f'PoseScorer: extra_layer.weight is {tuple(extra[0].shape)}, expected 1 to 1024 classes and a multiple of 4 features')
    return dict(convs=convs, extra=extra, widths=tuple(widths), classes=extra[0].shape[0])


class PoseScorer(torch.nn.Module):
    def __init__(self, path=None, state_dict=None, crop=CROP):
        super().__init__()
        if not isinstance(crop, int) or crop < 1:
            raise ValueError(f'PoseScorer: crop must be a positive integer, got {crop!r}')
        state_dict, path = resolve(path, state_dict, 'PoseScorer', 'pose classifier weight')
        net = parse_state_dict(state_dict, path)
        self.crop, self.widths, self.classes = crop, net['widths'], net['classes']
        self._spec = {}
        for i, (key, _, stride, pad, _) in enumerate(pose_conv_keys()):
            self._spec[key] = (i, stride, (pad, pad))
            self.register_buffer(f'w{i}', net['convs'][key][0])
            self.register_buffer(f'b{i}', net['convs'][key][1])
        self.register_buffer('extra_w', net['extra'][0])
        self.register_buffer('extra_b', net['extra'][1])
        self.eval()
        if torch.cuda.is_available():
            self.to('cuda')

    def _conv(self, key, x, act, res=None):
        i, stride, pad = self._spec[key]
        w, b = getattr(self, f'w{i}'), getattr(self, f'b{i}')
        if res is None:
            return _lib.conv2d(x, w, b, stride, pad, act=act)
        return _lib.conv2d_res(x, w, b, res, stride, pad, act=act)

    def _features(self, images, preprocessed):
        """[B,3,S,S] -> the pooled features [B,widths[3]].  An activation is dropped once its last reader has run: a block's input lives
        until the residual add, conv1's output until conv2 has read it."""
        check_images(images, 'PoseScorer', '[B,3,S,S]', square=True)
        S = images.shape[2]
        if S < self.crop or (S - self.crop) % 2:
            raise ValueError(f'PoseScorer: the {self.crop} px centre crop needs S >= {self.crop} with S - {self.crop} even, got {S}')
        if not images.is_cuda:
            raise RuntimeError(_NO_GPU)
        a = _lib.pose_stem_fwd(images.detach().float(), self.w0, self.b0, self.crop, preprocessed)
        a = _lib.maxpool3s2p1(a)
        for at, layer in enumerate(LAYERS):
            for blk in (0, 1):
                n = f'backbone.{layer}.{blk}'
                t = self._conv(f'{n}.conv1', a, 1)
                if at > 0 and blk == 0:
                    a = self._conv(f'{n}.downsample.0', a, 0)
                a = self._conv(f'{n}.conv2', t, 1, res=a)
                del t
        return _lib.adaptive_avgpool(a, 1, 1).view(a.shape[0], -1)             # avgpool + torch.flatten(out, 1)

    @torch.no_grad()
    def forward(self, images, preprocessed=False):
        """[B,3,S,S] RGB in [-1, 1] (preprocessed=True: BGR in [0, 255]) -> [B] fp32 on the device: p_0"""
        return _lib.cls_score(self._features(images, preprocessed), self.extra_w, self.extra_b, _lib.CLS_FIRST)

    @torch.no_grad()
    def probabilities(self, images, preprocessed=False):
        """-> [B,C] fp32 on the device: the softmax over the classes"""
        return _lib.cls_score(self._features(images, preprocessed), self.extra_w, self.extra_b, _lib.CLS_FIRST, want_prob=True)[1]


# ------------------------------------------------------------------------------------------------------------------------ CLI
def build_parser():
    parser = scorer_parser('score sampled images with the ResNet-18 pose classifier and fit the z+ and p+ editing boundaries '
                           '(edit_all_noinversion_ffhq.py:103-166 with --attribute_name pose)',
                           "the ClassifyModel state dict in the reference's layout (pth/classifier/pose/weight.pkl)")
    parser.add_argument('--crop', type=int, default=CROP, help='side of the centre crop')
    return parser


def main(argv=None):
    def make_scorer(args):
        scorer = PoseScorer(args.weights, crop=args.crop)
        return scorer, {'attribute': 'pose'}, {'classes': scorer.classes, 'crop': scorer.crop, 'widths': list(scorer.widths)}
    return scorer_main(build_parser(), argv, _NO_GPU, make_scorer)


if __name__ == '__main__':
    main(sys.argv[1:])
