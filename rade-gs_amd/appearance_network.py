"""The reference's per-view appearance CNN (scene/appearance_network.py), SURVEY 8f N8.

Same constructor arguments, sub-module names and default initialisation as upstream, so a state dict moves between the two with
strict=True:  conv1 (C_in -> 256), up1..up4 (pixel shuffle x2 + 3x3 conv + ReLU: 64 -> 128, 32 -> 64, 16 -> 32, 8 -> 16), a x2 bilinear
up-sampling (align_corners=True), conv2 (16 -> 16), conv3 (16 -> C_out), sigmoid.

`forward` is plain torch: it returns the mapping image as upstream does and is not the training path.  Training goes through
loss_utils.l1_loss_appearance, which runs conv1 and the four blocks of this module (at most half resolution) in torch and everything
after them -- the up-sampling, conv2, conv3, the product with the image and the L1 mean -- in the HIP head kernels."""
import torch
import torch.nn as nn
import torch.nn.functional as F


class UpsampleBlock(nn.Module):
    def __init__(self, num_input_channels, num_output_channels):
        super().__init__()
        self.pixel_shuffle = nn.PixelShuffle(2)
        self.conv = nn.Conv2d(num_input_channels // (2 * 2), num_output_channels, 3, stride=1, padding=1)
        self.relu = nn.ReLU()

    def forward(self, x):
        return self.relu(self.conv(self.pixel_shuffle(x)))


class AppearanceNetwork(nn.Module):
    def __init__(self, num_input_channels, num_output_channels):
        super().__init__()
        self.conv1 = nn.Conv2d(num_input_channels, 256, 3, stride=1, padding=1)
        self.up1 = UpsampleBlock(256, 128)
        self.up2 = UpsampleBlock(128, 64)
        self.up3 = UpsampleBlock(64, 32)
        self.up4 = UpsampleBlock(32, 16)
        self.conv2 = nn.Conv2d(16, 16, 3, stride=1, padding=1)
        self.conv3 = nn.Conv2d(16, num_output_channels, 3, stride=1, padding=1)
        self.relu = nn.ReLU()
        self.sigmoid = nn.Sigmoid()

    def trunk(self, x):
        """conv1 and the four blocks: [1,C_in,h,w] -> [1,16,16h,16w], the input of the full-resolution head"""
        return self.up4(self.up3(self.up2(self.up1(self.relu(self.conv1(x))))))

    def forward(self, x):
        x = F.interpolate(self.trunk(x), scale_factor=2, mode="bilinear", align_corners=True)
        return self.sigmoid(self.conv3(self.relu(self.conv2(x))))

    @classmethod
    def adopt(cls, module):
        """An AppearanceNetwork over the Parameter objects of `module` (any module with upstream's structure, e.g. the reference's own
        class after GaussianModel.training_setup): nothing is copied, so an optimizer group built on `module` keeps stepping the
        parameters this network reads."""
        names = ("conv1", "up1.conv", "up2.conv", "up3.conv", "up4.conv", "conv2", "conv3")
        convs = []
        for n in names:
            m = module
            for part in n.split("."):
                m = getattr(m, part, None)
            if not isinstance(m, nn.Conv2d):
                raise TypeError(f"adopt: `{n}` of {type(module).__name__} is not a Conv2d")
            convs.append(m)
        net = cls.__new__(cls)
        nn.Module.__init__(net)
        net.conv1 = convs[0]
        for i in range(4):
            blk = UpsampleBlock.__new__(UpsampleBlock)
            nn.Module.__init__(blk)
            blk.pixel_shuffle, blk.conv, blk.relu = nn.PixelShuffle(2), convs[1 + i], nn.ReLU()
            setattr(net, f"up{i + 1}", blk)
        net.conv2, net.conv3 = convs[5], convs[6]
        net.relu, net.sigmoid = nn.ReLU(), nn.Sigmoid()
        net.train(module.training)
        return net
