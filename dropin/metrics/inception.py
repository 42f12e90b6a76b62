"""metrics/inception.py:16-163 of the reference: `InceptionV3` with the reference's constructor signature, on the gfx950 kernels.
metrics/calc_inception.py:55 and metrics/fid_query.py:154 build it as InceptionV3([3], normalize_input=False) and read
`inception(img)[0].view(B, -1)`.  Only that use exists here: the pool3 block of the FID network."""
import torch

from transeditor_amd.inception_features import InceptionV3Features


class InceptionV3(torch.nn.Module):
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True):
        super().__init__()
        if list(output_blocks) != [3]:
            raise ValueError(f'InceptionV3: only output_blocks=[3] (the final average pool) exists here, got {list(output_blocks)}')
        if not use_fid_inception:
            raise ValueError("InceptionV3: only the FID network (use_fid_inception=True) exists here, not torchvision's")
        if requires_grad:
            raise ValueError('InceptionV3: the network is forward only here (requires_grad=False)')
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.output_blocks, self.last_needed_block = [3], 3
        self.net = InceptionV3Features(resize_input=resize_input)              # the weights: the torch hub cache path

    @torch.no_grad()
    def forward(self, inp):
        """[B,3,H,W] -> [features [B,2048,1,1]]; normalize_input=True takes (0, 1) images and applies 2 x - 1 first"""
        x = 2 * inp - 1 if self.normalize_input else inp
        return [self.net(x).view(inp.shape[0], 2048, 1, 1)]
