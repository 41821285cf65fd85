from . import drn, mobilenet, resnet, xception

# What the rest of the generator needs to know about a backbone:
#   tree           (output_stride, BatchNorm) -> its parameter tree
#   exec           (engine, output_stride) -> its execution on that engine's kernels; carries c_high / c_low, the channel counts of
#                  the high-level (ASPP input, aspp.py:37-42) and low-level (decoder input, decoder.py:11-16) features
#   transnorm      built with TransNorm (sync_bn=False) or not
#   output_stride  forced value, None: as asked for (deeplabv3.py:14-15: DRN's output sits at 1/8 whatever is asked for)
#   root           the child of the tree that holds the parameters the engine addresses as ``backbone.<root>.*`` ('' : the tree)
BACKBONES = {
    'mobilenet': dict(tree=mobilenet.MobileNetV2, exec=mobilenet.MobileNetV2Exec, transnorm=True, output_stride=None, root='features'),
    'resnet': dict(tree=resnet.ResNet101, exec=resnet.ResNetExec, transnorm=True, output_stride=None, root=''),
    'xception': dict(tree=xception.AlignedXception, exec=xception.XceptionExec, transnorm=False, output_stride=None, root=''),
    'drn': dict(tree=lambda output_stride, BatchNorm: drn.drn_d_54(BatchNorm), exec=drn.DRNExec, transnorm=False, output_stride=8,
                root=''),
}


def backbone_info(backbone):
    if backbone not in BACKBONES:
        raise NotImplementedError("backbone %r is not built (mobilenet, resnet, xception and drn are)" % (backbone,))
    return BACKBONES[backbone]


def build_backbone(backbone, output_stride, BatchNorm):
    return backbone_info(backbone)['tree'](output_stride, BatchNorm)
