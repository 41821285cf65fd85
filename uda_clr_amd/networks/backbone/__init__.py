from . import drn, mobilenet, resnet, xception


def build_backbone(backbone, output_stride, BatchNorm):
    if backbone == 'mobilenet':
        return mobilenet.MobileNetV2(output_stride, BatchNorm)
    if backbone == 'resnet':
        return resnet.ResNet101(output_stride, BatchNorm)
    if backbone == 'xception':
        return xception.AlignedXception(output_stride, BatchNorm)
    if backbone == 'drn':
        return drn.drn_d_54(BatchNorm)
    raise NotImplementedError("backbone %r is not built (mobilenet, resnet, xception and drn are)" % (backbone,))
