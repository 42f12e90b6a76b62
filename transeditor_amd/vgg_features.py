"""VGG16 fc7 features on the gfx950 kernels: the feature extractor of the reference's metrics/calc_prdc.py:101-104 (torchvision
`vgg16(pretrained=True)` with `classifier = classifier[:-1]`, in eval mode: the 4096-d output of fc7 after its ReLU).

    vgg = VGG16Features('vgg16-397923af.pth')                     # the file a user already has for LPIPS
    f = vgg(images)                                               # [B,3,H,W] in [-1, 1] -> [B,4096]
    evaluate_prdc(G, vgg, real_features)                          # an instance is a feature_fn of transeditor_amd.prdc

Weights come from a local torchvision vgg16 state dict (features.{0,...,28}.{weight,bias} and classifier.{0,3}.{weight,bias};
classifier.6.*, the ImageNet logits, is ignored).  Nothing is downloaded and torchvision is not imported.  As in the reference the
image goes into conv1_1 as it is: no ImageNet mean / std and none of LPIPS's scaling layer.

Layers: te_vgg_stem_fwd_f32 (conv1_1 + ReLU), conv1_2 ... conv5_3 on the project's 3x3 convolution with the max-pools of
csrc/lpips.hip between them (the trunk PerceptualLoss runs), pool5, te_adaptive_avgpool_f32 to 7 x 7 (the identity at 224 px,
overlapping 2 x 2 windows at 256 px), then fc6 and fc7 as te_fc_stream_f32 with bias and ReLU in its second pass.  Eval only: the two
Dropout layers are the identity and there is no backward pass.

Cost: the convolution trunk is nearly all of it (about 2.5 TFLOP per batch of 64 at 256 px against 15 GFLOP in fc6 + fc7); the fc
kernels exist so that the extractor exists, not to make the metric faster.  Measured shares: profiles/README.md.
"""
import torch

from . import _lib
from .frozen_net import VGGTrunk, check_images, no_gpu, resolve, weight_bias
from .lpips import default_vgg_path, vgg16_convs

FC_SHAPES = ((0, 4096, 512 * 7 * 7), (3, 4096, 4096))        # (index in vgg16.classifier, out features, in features): fc6, fc7


def vgg16_classifier(sd, path):
    """[(weight [J,K], bias [J])] for fc6 and fc7 from a torchvision vgg16 state dict (classifier.6.* ignored)"""
    return [weight_bias(sd, f'classifier.{idx}.weight', f'classifier.{idx}.bias', (j, k), 'VGG16Features', path,
                        'not a full torchvision vgg16 state dict') for idx, j, k in FC_SHAPES]


class VGG16Features(VGGTrunk, torch.nn.Module):
    def __init__(self, vgg_path=None, state_dict=None):
        super().__init__()
        if state_dict is None and vgg_path is None:
            vgg_path = default_vgg_path()
        state_dict, path = resolve(vgg_path, state_dict, 'VGG16Features', 'vgg16', arg='vgg_path')
        convs, fcs = vgg16_convs(state_dict, path, who='VGG16Features'), vgg16_classifier(state_dict, path)
        self._freeze(convs, [(f'fc{n}_{t}', v) for n, wb in zip((6, 7), fcs) for t, v in zip('wb', wb)])

    @torch.no_grad()
    def forward(self, images):
        """[B,3,H,W] in [-1, 1] -> [B,4096] fp32 on the device; H and W multiples of 32.  An activation is dropped once the next layer
        has read it."""
        check_images(images, 'VGG16Features')
        if images.shape[2] % 32 or images.shape[3] % 32 or images.shape[2] < 32 or images.shape[3] < 32:
            raise ValueError(f'VGG16Features: H and W must be multiples of 32, got {images.shape[2]}x{images.shape[3]}')
        if not images.is_cuda:
            raise RuntimeError(no_gpu('VGG16Features'))
        a = self._walk(lambda: _lib.vgg_stem_fwd(images.detach().float(), self._w(0), self.b0))
        a = _lib.maxpool2_fwd(a)                                               # features[30]
        a = _lib.adaptive_avgpool(a, 7, 7).view(a.shape[0], -1)                # avgpool + flatten
        a = _lib.fc_stream(a, self.fc6_w, self.fc6_b, act=1)                   # classifier[0:3] (Dropout: identity)
        return _lib.fc_stream(a, self.fc7_w, self.fc7_b, act=1)                # classifier[3:6]
