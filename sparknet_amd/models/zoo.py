"""Model zoo built with the DSL — the architectures SparkNet trains or BASELINE.json names:

* ``lenet``          — caffe/examples/mnist/lenet_train_test.prototxt
* ``cifar10_quick``  — caffe/examples/cifar10/cifar10_quick_train_test.prototxt
* ``cifar10_full``   — caffe/examples/cifar10/cifar10_full_train_test.prototxt (CifarApp)
* ``caffenet``       — caffe/models/bvlc_reference_caffenet/train_val.prototxt (ImageNetApp)
* ``alexnet``        — caffe/models/bvlc_alexnet/train_val.prototxt (LRN before pooling)
* ``googlenet``      — caffe/models/bvlc_googlenet/train_val.prototxt (aux heads 0.3)
* ``vgg16``          — not in the reference; authored here (BASELINE config #5)
* ``resnet50``       — not in the reference; the public Caffe ResNet-50 layout (conv without bias ->
  BatchNorm -> Scale -> ReLU blocks, Eltwise SUM shortcuts)
* ``resnet_cifar``   — not in the reference; the 6n+2-layer CIFAR ResNet from the same constructors
* ``mobilenet``      — not in the reference; the public Caffe MobileNet v1 layout (depthwise 3x3 +
  pointwise 1x1 blocks, each conv followed by BatchNorm -> Scale -> ReLU)
* ``resnext50``      — not in the reference; ResNeXt-50 32x4d (Xie et al. 2017): ResNet-50's stem and
  head around bottlenecks whose 3x3 is a 32-group convolution carrying the stage's stride
* ``mnasnet``        — not in the reference; MnasNet-B1 (Tan et al. 2019): inverted residuals whose depthwise
  layers are 3x3 or 5x5, each conv followed by BatchNorm -> Scale [-> ReLU]
* ``shufflenet``     — not in the reference; ShuffleNet v1 (Zhang et al. 2018): units of grouped 1x1, ShuffleChannel,
  depthwise 3x3 and grouped 1x1, summed with the input or concatenated with its average pooling
* ``fcn8s``          — not in the reference; FCN-8s (Long et al. 2015): the VGG-16 trunk, convolutional fc6 / fc7,
  three depthwise Deconvolution upsamplings fused with cropped pool4 / pool3 scores
* ``fast_rcnn``      — not in the reference; Fast R-CNN (Girshick 2015) on the CaffeNet or VGG-16 trunk: ROIPooling
  (or ROIAlign) of conv5 over given ROIs, fc6 / fc7, a SoftmaxWithLoss and a SmoothL1Loss head
* ``faster_rcnn``    — not in the reference; Faster R-CNN (Ren et al. 2015): the same trunks under a region-proposal
  network; TRAIN is the stage-1 RPN net, TEST runs the Proposal layer (decode, top-k, NMS) into ROIPooling and the head
* ``lrcn``           — not in the reference; LRCN (Donahue et al. 2015): the CaffeNet trunk through fc6 on every
  frame, one LSTM (fused step kernels) over the T frames of a stream and a per-timestep classifier
* ``se_resnet50``    — not in the reference; SE-ResNet-50 (Hu et al. 2018): ResNet-50 with a squeeze-and-
  excitation tail per block (global pool, two 1x1 convolutions, Sigmoid) gating the block output in an Axpy

Each builder returns a NetParameter whose data entry points are SparkNet ``JavaData``
layers (TRAIN and TEST variants, like ProtoLoader.replaceDataLayers), and each has a
matching ``*_solver`` with the reference hyper-parameters.
"""
from __future__ import annotations

from .. import proto
from ..dsl import (AccuracyLayer, AxpyLayer, BatchNormLayer, ConcatLayer, ConvolutionLayer, DropoutLayer, EltwiseLayer,
                   Include, InnerProductLayer, LRNLayer, NetParam, Pooling, PoolingLayer, RDDLayer, ReLULayer,
                   ScaleLayer, ShuffleChannelLayer, SigmoidLayer, SoftmaxWithLoss, CropLayer, DeconvolutionLayer,
                   ROIAlignLayer, ROIPoolingLayer, SmoothL1LossLayer, ProposalLayer, ReshapeLayer, SoftmaxLayer, LSTMLayer)
from ..ops.spec import PoolSpec

WB = [(1.0, 1.0), (2.0, 0.0)]   # weight / bias lr & decay mults used by the ImageNet models
W12 = [{"lr_mult": 1.0}, {"lr_mult": 2.0}]


def _g(std):
    return {"type": "gaussian", "std": std}


def _c(v=0.0):
    return {"type": "constant", "value": v}


XAV = {"type": "xavier"}


def data_layers(train_batch, test_batch, c, h, w):
    return [RDDLayer("data", [train_batch, c, h, w], Include.Train),
            RDDLayer("label", [train_batch, 1], Include.Train),
            RDDLayer("data", [test_batch, c, h, w], Include.Test),
            RDDLayer("label", [test_batch, 1], Include.Test)]


def _conv(name, bottom, k, n, stride=1, pad=0, group=1, wf=None, bf=None, param=WB):
    return ConvolutionLayer(name, [bottom], (k, k), n, stride=stride if stride != 1 else None,
                            pad=pad if pad else None, group=group, weight_filler=wf, bias_filler=bf, param=param)


def _relu(name, blob):
    return ReLULayer(name, [blob], in_place=True)


def _pool(name, bottom, k, s, ave=False, pad=0):
    return PoolingLayer(name, [bottom], Pooling.Ave if ave else Pooling.Max, (k, k), (s, s), pad=pad or None)


def _ip(name, bottom, n, wf, bf, param=WB):
    return InnerProductLayer(name, [bottom], n, weight_filler=wf, bias_filler=bf, param=param)


def _head(logits, top5=False, prefix=""):
    out = [AccuracyLayer(prefix + "accuracy", [logits, "label"])]
    if top5:
        out.append(AccuracyLayer(prefix + "accuracy_top5", [logits, "label"], top_k=5))
    out.append(SoftmaxWithLoss(prefix + "loss", [logits, "label"]))
    return out


# --------------------------------------------------------------------------------------

def lenet(train_batch=64, test_batch=100):
    return NetParam("LeNet", *data_layers(train_batch, test_batch, 1, 28, 28),
                    _conv("conv1", "data", 5, 20, wf=XAV, bf=_c(), param=W12),
                    _pool("pool1", "conv1", 2, 2),
                    _conv("conv2", "pool1", 5, 50, wf=XAV, bf=_c(), param=W12),
                    _pool("pool2", "conv2", 2, 2),
                    _ip("ip1", "pool2", 500, XAV, _c(), W12),
                    _relu("relu1", "ip1"),
                    _ip("ip2", "ip1", 10, XAV, _c(), W12),
                    *_head("ip2"))


def cifar10_quick(train_batch=100, test_batch=100):
    return NetParam("CIFAR10_quick", *data_layers(train_batch, test_batch, 3, 32, 32),
                    _conv("conv1", "data", 5, 32, pad=2, wf=_g(1e-4), bf=_c(), param=W12),
                    _pool("pool1", "conv1", 3, 2),
                    _relu("relu1", "pool1"),
                    _conv("conv2", "pool1", 5, 32, pad=2, wf=_g(0.01), bf=_c(), param=W12),
                    _relu("relu2", "conv2"),
                    _pool("pool2", "conv2", 3, 2, ave=True),
                    _conv("conv3", "pool2", 5, 64, pad=2, wf=_g(0.01), bf=_c(), param=W12),
                    _relu("relu3", "conv3"),
                    _pool("pool3", "conv3", 3, 2, ave=True),
                    _ip("ip1", "pool3", 64, _g(0.1), _c(), W12),
                    _ip("ip2", "ip1", 10, _g(0.1), _c(), W12),
                    *_head("ip2"))


def cifar10_full(train_batch=100, test_batch=100):
    return NetParam("CIFAR10_full", *data_layers(train_batch, test_batch, 3, 32, 32),
                    _conv("conv1", "data", 5, 32, pad=2, wf=_g(1e-4), bf=_c(), param=W12),
                    _pool("pool1", "conv1", 3, 2),
                    _relu("relu1", "pool1"),
                    LRNLayer("norm1", ["pool1"], 3, 5e-5, 0.75, within=True),
                    _conv("conv2", "norm1", 5, 32, pad=2, wf=_g(0.01), bf=_c(), param=W12),
                    _relu("relu2", "conv2"),
                    _pool("pool2", "conv2", 3, 2, ave=True),
                    LRNLayer("norm2", ["pool2"], 3, 5e-5, 0.75, within=True),
                    _conv("conv3", "norm2", 5, 64, pad=2, wf=_g(0.01), bf=_c(), param=None),
                    _relu("relu3", "conv3"),
                    _pool("pool3", "conv3", 3, 2, ave=True),
                    _ip("ip1", "pool3", 10, _g(0.01), _c(), [(1.0, 250.0), (2.0, 0.0)]),
                    *_head("ip1"))


def _fc_tail(bottom, drop=0.5, classes=1000):
    return [_ip("fc6", bottom, 4096, _g(0.005), _c(1.0)), _relu("relu6", "fc6"), DropoutLayer("drop6", ["fc6"], drop),
            _ip("fc7", "fc6", 4096, _g(0.005), _c(1.0)), _relu("relu7", "fc7"), DropoutLayer("drop7", ["fc7"], drop),
            _ip("fc8", "fc7", classes, _g(0.01), _c(0.0))]


def caffenet(train_batch=256, test_batch=50, crop=227, classes=1000):
    """bvlc_reference_caffenet: conv -> relu -> pool -> LRN ordering (ImageNetApp model)."""
    return NetParam("CaffeNet", *data_layers(train_batch, test_batch, 3, crop, crop),
                    _conv("conv1", "data", 11, 96, stride=4, wf=_g(0.01), bf=_c(0.0)),
                    _relu("relu1", "conv1"), _pool("pool1", "conv1", 3, 2),
                    LRNLayer("norm1", ["pool1"], 5, 1e-4, 0.75),
                    _conv("conv2", "norm1", 5, 256, pad=2, group=2, wf=_g(0.01), bf=_c(1.0)),
                    _relu("relu2", "conv2"), _pool("pool2", "conv2", 3, 2),
                    LRNLayer("norm2", ["pool2"], 5, 1e-4, 0.75),
                    _conv("conv3", "norm2", 3, 384, pad=1, wf=_g(0.01), bf=_c(0.0)), _relu("relu3", "conv3"),
                    _conv("conv4", "conv3", 3, 384, pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu4", "conv4"),
                    _conv("conv5", "conv4", 3, 256, pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu5", "conv5"),
                    _pool("pool5", "conv5", 3, 2),
                    *_fc_tail("pool5", classes=classes), *_head("fc8"))


def alexnet(train_batch=256, test_batch=50, crop=227, classes=1000):
    """bvlc_alexnet: conv -> relu -> LRN -> pool ordering."""
    return NetParam("AlexNet", *data_layers(train_batch, test_batch, 3, crop, crop),
                    _conv("conv1", "data", 11, 96, stride=4, wf=_g(0.01), bf=_c(0.0)),
                    _relu("relu1", "conv1"), LRNLayer("norm1", ["conv1"], 5, 1e-4, 0.75),
                    _pool("pool1", "norm1", 3, 2),
                    _conv("conv2", "pool1", 5, 256, pad=2, group=2, wf=_g(0.01), bf=_c(0.1)),
                    _relu("relu2", "conv2"), LRNLayer("norm2", ["conv2"], 5, 1e-4, 0.75),
                    _pool("pool2", "norm2", 3, 2),
                    _conv("conv3", "pool2", 3, 384, pad=1, wf=_g(0.01), bf=_c(0.0)), _relu("relu3", "conv3"),
                    _conv("conv4", "conv3", 3, 384, pad=1, group=2, wf=_g(0.01), bf=_c(0.1)), _relu("relu4", "conv4"),
                    _conv("conv5", "conv4", 3, 256, pad=1, group=2, wf=_g(0.01), bf=_c(0.1)), _relu("relu5", "conv5"),
                    _pool("pool5", "conv5", 3, 2),
                    *_fc_tail("pool5", classes=classes), *_head("fc8"))


INCEPTION = {  # name: (1x1, 3x3_reduce, 3x3, 5x5_reduce, 5x5, pool_proj)
    "3a": (64, 96, 128, 16, 32, 32), "3b": (128, 128, 192, 32, 96, 64),
    "4a": (192, 96, 208, 16, 48, 64), "4b": (160, 112, 224, 24, 64, 64),
    "4c": (128, 128, 256, 24, 64, 64), "4d": (112, 144, 288, 32, 64, 64),
    "4e": (256, 160, 320, 32, 128, 128), "5a": (256, 160, 320, 32, 128, 128),
    "5b": (384, 192, 384, 48, 128, 128),
}
B02 = _c(0.2)


def _inception(name, bottom):
    n1, r3, n3, r5, n5, pp = INCEPTION[name]
    p = f"inception_{name}/"
    L = []
    for suffix, k, n, src, pad in (("1x1", 1, n1, bottom, 0), ("3x3_reduce", 1, r3, bottom, 0),
                                   ("3x3", 3, n3, p + "3x3_reduce", 1), ("5x5_reduce", 1, r5, bottom, 0),
                                   ("5x5", 5, n5, p + "5x5_reduce", 2)):
        L += [_conv(p + suffix, src, k, n, pad=pad, wf=XAV, bf=B02), _relu(p + "relu_" + suffix, p + suffix)]
    L += [_pool(p + "pool", bottom, 3, 1, pad=1),
          _conv(p + "pool_proj", p + "pool", 1, pp, wf=XAV, bf=B02), _relu(p + "relu_pool_proj", p + "pool_proj"),
          ConcatLayer(p + "output", [p + "1x1", p + "3x3", p + "5x5", p + "pool_proj"])]
    return L, p + "output"


def _aux(idx, bottom, classes):
    p = f"loss{idx}/"
    return [_pool(p + "ave_pool", bottom, 5, 3, ave=True),
            _conv(p + "conv", p + "ave_pool", 1, 128, wf=XAV, bf=B02), _relu(p + "relu_conv", p + "conv"),
            _ip(p + "fc", p + "conv", 1024, XAV, B02), _relu(p + "relu_fc", p + "fc"),
            DropoutLayer(p + "drop_fc", [p + "fc"], 0.7),
            _ip(p + "classifier", p + "fc", classes, XAV, _c(0.0)),
            SoftmaxWithLoss(p + "loss", [p + "classifier", "label"], loss_weight=0.3, top=[p + f"loss{idx}"]),
            AccuracyLayer(p + "top-1", [p + "classifier", "label"]),
            AccuracyLayer(p + "top-5", [p + "classifier", "label"], top_k=5)]


def googlenet(train_batch=32, test_batch=50, crop=224, classes=1000, aux=True):
    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    L += [_conv("conv1/7x7_s2", "data", 7, 64, stride=2, pad=3, wf=XAV, bf=B02), _relu("conv1/relu_7x7", "conv1/7x7_s2"),
          _pool("pool1/3x3_s2", "conv1/7x7_s2", 3, 2), LRNLayer("pool1/norm1", ["pool1/3x3_s2"], 5, 1e-4, 0.75),
          _conv("conv2/3x3_reduce", "pool1/norm1", 1, 64, wf=XAV, bf=B02),
          _relu("conv2/relu_3x3_reduce", "conv2/3x3_reduce"),
          _conv("conv2/3x3", "conv2/3x3_reduce", 3, 192, pad=1, wf=XAV, bf=B02), _relu("conv2/relu_3x3", "conv2/3x3"),
          LRNLayer("conv2/norm2", ["conv2/3x3"], 5, 1e-4, 0.75), _pool("pool2/3x3_s2", "conv2/norm2", 3, 2)]
    x = "pool2/3x3_s2"
    for name in ("3a", "3b"):
        m, x = _inception(name, x)
        L += m
    L.append(_pool("pool3/3x3_s2", x, 3, 2))
    x = "pool3/3x3_s2"
    for name in ("4a", "4b", "4c", "4d", "4e"):
        m, x = _inception(name, x)
        L += m
        if aux and name == "4a":
            L += _aux(1, x, classes)
        if aux and name == "4d":
            L += _aux(2, x, classes)
    L.append(_pool("pool4/3x3_s2", x, 3, 2))
    x = "pool4/3x3_s2"
    for name in ("5a", "5b"):
        m, x = _inception(name, x)
        L += m
    L += [_pool("pool5/7x7_s1", x, 7, 1, ave=True), DropoutLayer("pool5/drop_7x7_s1", ["pool5/7x7_s1"], 0.4),
          _ip("loss3/classifier", "pool5/7x7_s1", classes, XAV, _c(0.0)),
          SoftmaxWithLoss("loss3/loss3", ["loss3/classifier", "label"], loss_weight=1.0),
          AccuracyLayer("loss3/top-1", ["loss3/classifier", "label"]),
          AccuracyLayer("loss3/top-5", ["loss3/classifier", "label"], top_k=5)]
    return NetParam("GoogleNet", *L)


def vgg16(train_batch=64, test_batch=50, crop=224, classes=1000):
    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x = "data"
    cfg = [(64, 2), (128, 2), (256, 3), (512, 3), (512, 3)]
    for stage, (n, reps) in enumerate(cfg, 1):
        for r in range(1, reps + 1):
            name = f"conv{stage}_{r}"
            L += [_conv(name, x, 3, n, pad=1, wf={"type": "msra"}, bf=_c(0.0)), _relu(f"relu{stage}_{r}", name)]
            x = name
        L.append(_pool(f"pool{stage}", x, 2, 2))
        x = f"pool{stage}"
    L += [_ip("fc6", x, 4096, _g(0.005), _c(0.1)), _relu("relu6", "fc6"), DropoutLayer("drop6", ["fc6"], 0.5),
          _ip("fc7", "fc6", 4096, _g(0.005), _c(0.1)), _relu("relu7", "fc7"), DropoutLayer("drop7", ["fc7"], 0.5),
          _ip("fc8", "fc7", classes, _g(0.01), _c(0.0)), *_head("fc8", top5=True)]
    return NetParam("VGG_ILSVRC_16_layers", *L)


def fcn8s(classes=21, train_batch=1, test_batch=1, crop=500, width=1.0):
    """FCN-8s (Long, Shelhamer, Darrell 2015, "Fully Convolutional Networks for Semantic Segmentation";
    layer names of the public voc-fcn8s net): not in the reference.  The VGG-16 trunk with ``conv1_1``
    padded by 100, ``fc6`` as a 7x7 and ``fc7`` as a 1x1 convolution with dropout, the class scores
    ``score_fr``, then three learned upsamplings — depthwise Deconvolution layers (group = classes, no
    bias, ``bilinear`` filler: csrc/kernels/conv_updw.hip): ``upscore2`` (4x4 / 2) fused (Eltwise SUM)
    with ``score_pool4`` cropped at offset 5, ``upscore_pool4`` (4x4 / 2) fused with ``score_pool3``
    cropped at offset 9, and ``upscore8`` (16x16 / 8, lr_mult 0) cropped against ``data`` at offset 31 to
    ``score``.  SoftmaxWithLoss over the channel axis with ignore_label 255, not normalised; the label
    is [N, 1, crop, crop].  ``width`` scales the trunk's channel counts (rounded to multiples of 8),
    ``fc6`` / ``fc7`` included.  At crop 500: fc6 16 x 16, upscore2 34, upscore_pool4 70, upscore8 568."""
    ch = lambda n: max(8, int(n * width / 8 + 0.5) * 8)
    L = [RDDLayer("data", [train_batch, 3, crop, crop], Include.Train),
         RDDLayer("label", [train_batch, 1, crop, crop], Include.Train),
         RDDLayer("data", [test_batch, 3, crop, crop], Include.Test),
         RDDLayer("label", [test_batch, 1, crop, crop], Include.Test)]
    x = "data"
    for stage, (n, reps) in enumerate([(64, 2), (128, 2), (256, 3), (512, 3), (512, 3)], 1):
        for r in range(1, reps + 1):
            name = f"conv{stage}_{r}"
            L += [_conv(name, x, 3, ch(n), pad=100 if x == "data" else 1, wf=MSRA, bf=_c(0.0)),
                  _relu(f"relu{stage}_{r}", name)]
            x = name
        L.append(_pool(f"pool{stage}", x, 2, 2))
        x = f"pool{stage}"
    L += [_conv("fc6", x, 7, ch(4096), wf=MSRA, bf=_c(0.0)), _relu("relu6", "fc6"), DropoutLayer("drop6", ["fc6"], 0.5),
          _conv("fc7", "fc6", 1, ch(4096), wf=MSRA, bf=_c(0.0)), _relu("relu7", "fc7"),
          DropoutLayer("drop7", ["fc7"], 0.5), _conv("score_fr", "fc7", 1, classes, wf=MSRA, bf=_c(0.0))]

    def up(name, bottom, f, lr):
        return DeconvolutionLayer(name, [bottom], (2 * f - f % 2,) * 2, classes, stride=f, group=classes,
                                  weight_filler={"type": "bilinear"}, param=[(lr, lr)], bias_term=False)

    def skip(pool, bottom, offset, fuse):
        L.extend([_conv(f"score_{pool}", pool, 1, classes, wf=MSRA, bf=_c(0.0)),
                  CropLayer(f"score_{pool}c", [f"score_{pool}", bottom], offset),
                  EltwiseLayer(fuse, [bottom, f"score_{pool}c"], "SUM")])
        return fuse

    L.append(up("upscore2", "score_fr", 2, 1.0))
    x = skip("pool4", "upscore2", 5, "fuse_pool4")
    L.append(up("upscore_pool4", x, 2, 1.0))
    x = skip("pool3", "upscore_pool4", 9, "fuse_pool3")
    loss = SoftmaxWithLoss("loss", ["score", "label"])
    loss.loss_param.ignore_label = 255
    loss.loss_param.normalize = False
    L += [up("upscore8", x, 8, 0.0), CropLayer("score", ["upscore8", "data"], 31), loss]
    return NetParam("voc-fcn8s", *L)


def _rcnn_trunk(who, trunk, ch, size):
    """The detection nets' trunk from ``data`` to ``conv5`` (CaffeNet) / ``conv5_3`` (VGG-16) without its last pool,
    its first layers frozen as published: (layers, top blob, ROI bins, the top's height = width for a ``size``
    square input)."""
    if trunk not in ("caffenet", "vgg16"):
        raise ValueError(f"{who}: trunk {trunk!r} is neither 'caffenet' nor 'vgg16'")
    frozen = [(0.0, 0.0), (0.0, 0.0)]
    half = lambda n, k: -(-(n - k) // 2) + 1  # a stride-2 pooling with Caffe's ceil
    L = []
    if trunk == "caffenet":
        L += [_conv("conv1", "data", 11, ch(96), stride=4, wf=_g(0.01), bf=_c(0.0), param=frozen),
              _relu("relu1", "conv1"), _pool("pool1", "conv1", 3, 2), LRNLayer("norm1", ["pool1"], 5, 1e-4, 0.75),
              _conv("conv2", "norm1", 5, ch(256), pad=2, group=2, wf=_g(0.01), bf=_c(1.0)),
              _relu("relu2", "conv2"), _pool("pool2", "conv2", 3, 2), LRNLayer("norm2", ["pool2"], 5, 1e-4, 0.75),
              _conv("conv3", "norm2", 3, ch(384), pad=1, wf=_g(0.01), bf=_c(0.0)), _relu("relu3", "conv3"),
              _conv("conv4", "conv3", 3, ch(384), pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu4", "conv4"),
              _conv("conv5", "conv4", 3, ch(256), pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu5", "conv5")]
        return L, "conv5", (6, 6), half(half((size - 11) // 4 + 1, 3), 3)
    x, side = "data", size
    for stage, (n, reps) in enumerate([(64, 2), (128, 2), (256, 3), (512, 3), (512, 3)], 1):
        for r in range(1, reps + 1):
            name = f"conv{stage}_{r}"
            L += [_conv(name, x, 3, ch(n), pad=1, wf=MSRA, bf=_c(0.0), param=frozen if stage <= 2 else WB),
                  _relu(f"relu{stage}_{r}", name)]
            x = name
        if stage < 5:
            L.append(_pool(f"pool{stage}", x, 2, 2))
            x, side = f"pool{stage}", half(side, 2)
    return L, x, (7, 7), side


def fast_rcnn(trunk="caffenet", classes=21, images=2, rois=128, size=600, align=False, width=1.0):
    """Fast R-CNN (Girshick 2015; layer and blob names of the public CaffeNet / VGG16 train nets): not in the
    reference.  Inputs ``data`` [images, 3, size, size], ``rois`` [rois, 5] as (image, x1, y1, x2, y2),
    ``labels`` [rois] and ``bbox_targets`` / ``bbox_inside_weights`` / ``bbox_outside_weights`` [rois, 4
    classes].  The trunk runs to ``conv5`` (CaffeNet) / ``conv5_3`` (VGG-16) without its last pool, its first
    layers frozen as published; ``roi_pool5`` is a ROIPooling (``align``: ROIAlign, 2 x 2 samples) of 6 x 6
    (7 x 7 for VGG-16) bins at scale 1 / 16 (csrc/kernels/roi.hip); ``fc6`` / ``fc7`` with dropout feed
    ``cls_score`` into ``loss_cls`` (SoftmaxWithLoss) and ``bbox_pred`` into ``loss_bbox`` (SmoothL1Loss).
    ``width`` scales the trunk's and the fc layers' channel counts (rounded to multiples of 8)."""
    ch = lambda n: max(8, int(n * width / 8 + 0.5) * 8)
    L = [RDDLayer("data", [images, 3, size, size]), RDDLayer("rois", [rois, 5]), RDDLayer("labels", [rois])]
    L += [RDDLayer(n, [rois, 4 * classes]) for n in ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights")]
    trunk_layers, x, pooled, _ = _rcnn_trunk("fast_rcnn", trunk, ch, size)
    L += trunk_layers
    L.append(ROIAlignLayer("roi_pool5", [x, "rois"], pooled, 1.0 / 16, 2) if align else
             ROIPoolingLayer("roi_pool5", [x, "rois"], pooled, 1.0 / 16))
    L += [_ip("fc6", "roi_pool5", ch(4096), _g(0.005), _c(0.1)), _relu("relu6", "fc6"), DropoutLayer("drop6", ["fc6"], 0.5),
          _ip("fc7", "fc6", ch(4096), _g(0.005), _c(0.1)), _relu("relu7", "fc7"), DropoutLayer("drop7", ["fc7"], 0.5),
          _ip("cls_score", "fc7", classes, _g(0.01), _c(0.0)), _ip("bbox_pred", "fc7", 4 * classes, _g(0.001), _c(0.0)),
          SoftmaxWithLoss("loss_cls", ["cls_score", "labels"], loss_weight=1.0),
          SmoothL1LossLayer("loss_bbox", ["bbox_pred", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights"],
                            loss_weight=1.0)]
    return NetParam("CaffeNet" if trunk == "caffenet" else "VGG_ILSVRC_16_layers", *L)


def _only(include, *layers):
    for lp in layers:
        lp.include.add().phase = proto.TRAIN if include is Include.Train else proto.TEST
    return list(layers)


def faster_rcnn(trunk="vgg16", classes=21, images=1, size=600, width=1.0, pre_nms_topn=6000, post_nms_topn=300,
                nms_thresh=0.7):
    """Faster R-CNN (Ren et al. 2015; layer and blob names of the public alternating-optimisation nets): not in
    the reference.  Inputs ``data`` [images, 3, size, size] and ``im_info`` [images, 3] = (height, width, scale).
    ``fast_rcnn``'s trunk feeds the region-proposal network: ``rpn_conv/3x3``, ``rpn_cls_score`` (18) and
    ``rpn_bbox_pred`` (36) for 9 anchors per conv5 pixel.  TRAIN is the stage-1 RPN training net with the anchor
    targets as inputs (``rpn_labels`` [images, 1, 9 H, W], ``rpn_bbox_targets`` and its inside / outside weights
    [images, 36, H, W]), ``rpn_loss_cls`` and ``rpn_loss_bbox``.  TEST is the detector: ``proposal``
    (csrc/kernels/proposal.hip) turns the RPN's outputs into ``images post_nms_topn`` ROIs, unused rows carrying
    image -1, for ``roi_pool5`` and the Fast R-CNN head.  ``width`` scales the channel counts."""
    ch = lambda n: max(8, int(n * width / 8 + 0.5) * 8)
    L, x, pooled, side = _rcnn_trunk("faster_rcnn", trunk, ch, size)
    L = [RDDLayer("data", [images, 3, size, size]), RDDLayer("im_info", [images, 3])] + L
    L += _only(Include.Train, RDDLayer("rpn_labels", [images, 1, 9 * side, side]),
               *[RDDLayer(n, [images, 36, side, side])
                 for n in ("rpn_bbox_targets", "rpn_bbox_inside_weights", "rpn_bbox_outside_weights")])
    L += [_conv("rpn_conv/3x3", x, 3, ch(512), pad=1, wf=_g(0.01), bf=_c(0.0)), _relu("rpn_relu/3x3", "rpn_conv/3x3"),
          _conv("rpn_cls_score", "rpn_conv/3x3", 1, 18, wf=_g(0.01), bf=_c(0.0)),
          _conv("rpn_bbox_pred", "rpn_conv/3x3", 1, 36, wf=_g(0.01), bf=_c(0.0)),
          ReshapeLayer("rpn_cls_score_reshape", ["rpn_cls_score"], [0, 2, -1, 0])]
    L += _only(Include.Train,
               SoftmaxWithLoss("rpn_loss_cls", ["rpn_cls_score_reshape", "rpn_labels"], loss_weight=1.0,
                               ignore_label=-1, normalize=True, top=["rpn_cls_loss"]),
               SmoothL1LossLayer("rpn_loss_bbox", ["rpn_bbox_pred", "rpn_bbox_targets", "rpn_bbox_inside_weights",
                                                   "rpn_bbox_outside_weights"], sigma=3.0, loss_weight=1.0,
                                 top=["rpn_loss_bbox"]))
    L += _only(Include.Test,
               SoftmaxLayer("rpn_cls_prob", ["rpn_cls_score_reshape"]),
               ReshapeLayer("rpn_cls_prob_reshape", ["rpn_cls_prob"], [0, 18, -1, 0]),
               ProposalLayer("proposal", ["rpn_cls_prob_reshape", "rpn_bbox_pred", "im_info"], top=["rois"],
                             pre_nms_topn=pre_nms_topn, post_nms_topn=post_nms_topn, nms_thresh=nms_thresh),
               ROIPoolingLayer("roi_pool5", [x, "rois"], pooled, 1.0 / 16),
               _ip("fc6", "roi_pool5", ch(4096), _g(0.005), _c(0.1)), _relu("relu6", "fc6"),
               DropoutLayer("drop6", ["fc6"], 0.5),
               _ip("fc7", "fc6", ch(4096), _g(0.005), _c(0.1)), _relu("relu7", "fc7"), DropoutLayer("drop7", ["fc7"], 0.5),
               _ip("cls_score", "fc7", classes, _g(0.01), _c(0.0)), _ip("bbox_pred", "fc7", 4 * classes, _g(0.001), _c(0.0)),
               SoftmaxLayer("cls_prob", ["cls_score"]))
    return NetParam("CaffeNet" if trunk == "caffenet" else "VGG_ILSVRC_16_layers", *L)


def lrcn(T=16, N=24, classes=101, size=227, width=1.0, drop=0.5, trunk=True):
    """LRCN (Donahue et al. 2015; layer and blob names of upstream's examples/LRCN_activity_recognition): not in
    the reference.  Inputs ``data`` [T N, 3, size, size] with frame t of stream n at row t N + n, ``label`` [T, N]
    and ``clip_markers`` [T, N] (0 where a stream starts, else 1).  The CaffeNet trunk through ``fc6`` runs on all
    T N frames at once; ``reshape-data`` makes them [T, N, 4096] for ``lstm1`` (256 units; the step kernels of
    csrc/kernels/lstm.hip), ``fc8-final`` classifies every timestep (axis 2) and the SoftmaxWithLoss takes the
    scores and labels flattened to T N rows.  ``width`` scales the channel counts and the LSTM's units.
    ``trunk=False`` is the recurrent head alone on stored fc6 features: ``fc6-reshape`` [T, N, 4096] is an input."""
    ch = lambda n: max(8, int(n * width / 8 + 0.5) * 8)
    fc8 = _ip("fc8-final", "lstm1", classes, _g(0.01), _c(0.0))
    fc8.inner_product_param.axis = 2
    head = [LSTMLayer("lstm1", ["fc6-reshape", "clip_markers"], ch(256),
                      weight_filler={"type": "uniform", "min": -0.01, "max": 0.01}, bias_filler=_c(0.0)),
            DropoutLayer("lstm1-drop", ["lstm1"], drop), fc8,
            ReshapeLayer("reshape-score", ["fc8-final"], [-1, classes], top=["score"]),
            ReshapeLayer("reshape-label", ["label"], [-1, 1], top=["label-flat"]),
            SoftmaxWithLoss("loss", ["score", "label-flat"])]
    if not trunk:
        return NetParam("lstm_joints", RDDLayer("fc6-reshape", [T, N, ch(4096)]), RDDLayer("label", [T, N]),
                        RDDLayer("clip_markers", [T, N]), *head)
    return NetParam("lstm_joints", RDDLayer("data", [T * N, 3, size, size]), RDDLayer("label", [T, N]),
                    RDDLayer("clip_markers", [T, N]),
                    _conv("conv1", "data", 11, ch(96), stride=4, wf=_g(0.01), bf=_c(0.0)),
                    _relu("relu1", "conv1"), _pool("pool1", "conv1", 3, 2), LRNLayer("norm1", ["pool1"], 5, 1e-4, 0.75),
                    _conv("conv2", "norm1", 5, ch(256), pad=2, group=2, wf=_g(0.01), bf=_c(1.0)),
                    _relu("relu2", "conv2"), _pool("pool2", "conv2", 3, 2), LRNLayer("norm2", ["pool2"], 5, 1e-4, 0.75),
                    _conv("conv3", "norm2", 3, ch(384), pad=1, wf=_g(0.01), bf=_c(0.0)), _relu("relu3", "conv3"),
                    _conv("conv4", "conv3", 3, ch(384), pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu4", "conv4"),
                    _conv("conv5", "conv4", 3, ch(256), pad=1, group=2, wf=_g(0.01), bf=_c(1.0)), _relu("relu5", "conv5"),
                    _pool("pool5", "conv5", 3, 2),
                    _ip("fc6", "pool5", ch(4096), _g(0.005), _c(1.0)), _relu("relu6", "fc6"),
                    DropoutLayer("drop6", ["fc6"], drop),
                    ReshapeLayer("reshape-data", ["fc6"], [T, N, -1], top=["fc6-reshape"]), *head)


MSRA = {"type": "msra"}
W1 = [(1.0, 1.0)]


def _conv_bn(L, name, bn, bottom, k, n, stride=1, pad=0, relu=True, group=1, names=None):
    """Bias-free convolution -> in-place BatchNorm -> in-place Scale (with bias) [-> in-place
    ReLU]: the chain engine.fuse_bn_scale_relu runs in one kernel family.  ``bn`` is the suffix
    of the bn* / scale* layer names (public ResNet naming); ``names`` = (BatchNorm, Scale, ReLU)
    layer names for models that name them differently."""
    bn_name, scale_name, relu_name = names or ("bn" + bn, "scale" + bn, name + "_relu")
    L += [ConvolutionLayer(name, [bottom], (k, k), n, stride=stride if stride != 1 else None, pad=pad or None,
                           group=group, weight_filler=MSRA, param=W1, bias_term=False),
          BatchNormLayer(bn_name, [name], in_place=True),
          ScaleLayer(scale_name, [name], in_place=True, bias_term=True)]
    if relu:
        L.append(_relu(relu_name, name))
    return name


def _bottleneck(L, tag, bottom, width, stride, project):
    """res{tag}: 1x1 (stride) -> 3x3 -> 1x1 (x4), summed with the input or its projection."""
    short = bottom
    if project:
        short = _conv_bn(L, f"res{tag}_branch1", f"{tag}_branch1", bottom, 1, 4 * width, stride=stride, relu=False)
    x = _conv_bn(L, f"res{tag}_branch2a", f"{tag}_branch2a", bottom, 1, width, stride=stride)
    x = _conv_bn(L, f"res{tag}_branch2b", f"{tag}_branch2b", x, 3, width, pad=1)
    x = _conv_bn(L, f"res{tag}_branch2c", f"{tag}_branch2c", x, 1, 4 * width, relu=False)
    L += [EltwiseLayer(f"res{tag}", [short, x], "SUM"), _relu(f"res{tag}_relu", f"res{tag}")]
    return f"res{tag}"


def resnet50(train_batch=32, test_batch=50, crop=224, classes=1000):
    """ResNet-50 in the layout of the public Caffe release (He et al., ResNet-50-deploy.prototxt):
    not in the reference; 25 557 032 learnable elements besides the BatchNorm statistics."""
    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x = _conv_bn(L, "conv1", "_conv1", "data", 7, 64, stride=2, pad=3)
    L.append(_pool("pool1", x, 3, 2))
    x = "pool1"
    for stage, (width, reps) in enumerate(((64, 3), (128, 4), (256, 6), (512, 3)), 2):
        for r in range(reps):
            x = _bottleneck(L, f"{stage}{chr(ord('a') + r)}", x, width, 2 if (r == 0 and stage > 2) else 1, r == 0)
    L += [PoolingLayer("pool5", [x], Pooling.Ave, global_pooling=True),
          _ip(f"fc{classes}", "pool5", classes, MSRA, _c(0.0)), *_head(f"fc{classes}", top5=True)]
    return NetParam("ResNet-50", *L)


def resnet_cifar(n=3, train_batch=128, test_batch=100, classes=10):
    """The 6n+2-layer CIFAR ResNet (He et al. 2015, section 4.2): 3x3 stem, three stages of n
    basic blocks at 16 / 32 / 64 channels, projection shortcuts where the shape changes."""
    L = list(data_layers(train_batch, test_batch, 3, 32, 32))
    x = _conv_bn(L, "conv1", "_conv1", "data", 3, 16, pad=1)
    for stage, width in enumerate((16, 32, 64), 2):
        for r in range(n):
            tag = f"{stage}{chr(ord('a') + r)}" if n <= 26 else f"{stage}_{r + 1}"
            stride = 2 if (r == 0 and stage > 2) else 1
            short = x
            if stride != 1:
                short = _conv_bn(L, f"res{tag}_branch1", f"{tag}_branch1", x, 1, width, stride=stride, relu=False)
            y = _conv_bn(L, f"res{tag}_branch2a", f"{tag}_branch2a", x, 3, width, stride=stride, pad=1)
            y = _conv_bn(L, f"res{tag}_branch2b", f"{tag}_branch2b", y, 3, width, pad=1, relu=False)
            L += [EltwiseLayer(f"res{tag}", [short, y], "SUM"), _relu(f"res{tag}_relu", f"res{tag}")]
            x = f"res{tag}"
    L += [PoolingLayer("pool_global", [x], Pooling.Ave, global_pooling=True),
          _ip("fc", "pool_global", classes, MSRA, _c(0.0), W12), *_head("fc")]
    return NetParam(f"ResNet-{6 * n + 2}-CIFAR", *L)


# (tag, output width, stride of the depthwise 3x3) of MobileNet v1's 13 depthwise-separable blocks
MOBILENET = (("2_1", 64, 1), ("2_2", 128, 2), ("3_1", 128, 1), ("3_2", 256, 2), ("4_1", 256, 1), ("4_2", 512, 2),
             ("5_1", 512, 1), ("5_2", 512, 1), ("5_3", 512, 1), ("5_4", 512, 1), ("5_5", 512, 1), ("5_6", 1024, 2),
             ("6", 1024, 1))


def mobilenet(train_batch=32, test_batch=50, crop=224, classes=1000, alpha=1.0):
    """MobileNet v1 (Howard et al. 2017) in the layout and layer names of the public Caffe
    release: not in the reference.  3x3 / 2 stem, 13 blocks of depthwise 3x3 (``convX/dw``,
    group == channels: csrc/kernels/conv_dw.hip) and pointwise 1x1 (``convX/sep``), each conv
    bias-free with in-place BatchNorm -> Scale -> ReLU, global average ``pool6`` (any crop) and
    ``fc7`` as a 1x1 convolution with bias.  4 231 976 learnable elements besides the BatchNorm
    statistics at alpha = 1.  ``alpha`` is the paper's width multiplier; widths stay multiples
    of 8 (the 16-byte channel lanes of the kernels)."""
    def width(n):
        return max(8, int(n * alpha + 4) // 8 * 8)

    def block(name, tag, bottom, k, n, **kw):
        return _conv_bn(L, name, None, bottom, k, n, names=(name + "/bn", name + "/scale", "relu" + tag), **kw)

    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x = block("conv1", "1", "data", 3, width(32), stride=2, pad=1)
    c = width(32)
    for tag, n, stride in MOBILENET:
        x = block(f"conv{tag}/dw", f"{tag}/dw", x, 3, c, stride=stride, pad=1, group=c)
        c = width(n)
        x = block(f"conv{tag}/sep", f"{tag}/sep", x, 1, c)
    L += [PoolingLayer("pool6", [x], Pooling.Ave, global_pooling=True),
          _conv("fc7", "pool6", 1, classes, wf=MSRA, bf=_c(0.0)), *_head("fc7", top5=True)]
    return NetParam("MobileNet", *L)


# (output width, depthwise window, stride, expansion, repeats) of MnasNet-B1's inverted-residual stacks
MNASNET = ((24, 3, 2, 3, 3), (40, 5, 2, 3, 3), (80, 5, 2, 6, 3), (96, 3, 1, 6, 2), (192, 5, 2, 6, 4), (320, 3, 1, 6, 1))


def mnasnet(train_batch=32, test_batch=50, crop=224, classes=1000, alpha=1.0):
    """MnasNet-B1 (Tan et al. 2019, "MnasNet: Platform-Aware Neural Architecture Search for Mobile"):
    not in the reference.  3x3 / 2 stem to 32 channels, a depthwise 3x3 and a 1x1 to 16, then the
    MNASNET stacks of inverted residuals — ``blockS_R/expand`` (1x1 to expansion x input width),
    ``/dw`` (depthwise 3x3: csrc/kernels/conv_dw.hip, or 5x5: csrc/kernels/conv_xdw.hip; carries the
    stride in a stack's first block; pad (window - 1) / 2) and ``/project`` (1x1, no ReLU), with an
    Eltwise SUM shortcut ``blockS_R`` where the stride is 1 and the width does not change — a 1x1 to
    1280, global average ``pool`` (any crop) and the InnerProduct ``fc`` with bias.  Every conv is
    bias-free with in-place BatchNorm -> Scale [-> ReLU].  4 383 312 learnable elements besides the
    BatchNorm statistics at alpha = 1, 1000 classes.  ``alpha`` is the width multiplier of every
    layer but the 1280-wide one; widths stay multiples of 8 (the 16-byte channel lanes of the kernels)."""
    def width(n):
        return max(8, int(n * alpha + 4) // 8 * 8)

    def block(name, bottom, k, n, **kw):
        return _conv_bn(L, name, None, bottom, k, n, names=(name + "/bn", name + "/scale", name + "/relu"), **kw)

    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    c = width(32)
    x = block("stem/conv", "data", 3, c, stride=2, pad=1)
    x = block("stem/dw", x, 3, c, pad=1, group=c)
    c = width(16)
    x = block("stem/sep", x, 1, c, relu=False)
    for stage, (n, k, stride, expansion, reps) in enumerate(MNASNET, 1):
        n = width(n)
        for r in range(1, reps + 1):
            tag, first = f"block{stage}_{r}", r == 1
            y = block(tag + "/expand", x, 1, c * expansion)
            y = block(tag + "/dw", y, k, c * expansion, stride=stride if first else 1, pad=(k - 1) // 2,
                      group=c * expansion)
            y = block(tag + "/project", y, 1, n, relu=False)
            if c == n and (stride == 1 or not first):
                L.append(EltwiseLayer(tag, [x, y], "SUM"))
                y = tag
            x, c = y, n
    x = block("head/conv", x, 1, 1280)
    L += [PoolingLayer("pool", [x], Pooling.Ave, global_pooling=True),
          _ip("fc", "pool", classes, MSRA, _c(0.0)), *_head("fc", top5=True)]
    return NetParam("MnasNet-B1", *L)


# widths of ShuffleNet v1's three stages by the number of groups (Zhang et al. 2018, table 1), and their units
SHUFFLENET_WIDTHS = {1: (144, 288, 576), 2: (200, 400, 800), 3: (240, 480, 960), 4: (272, 544, 1088),
                     8: (384, 768, 1536)}
SHUFFLENET_UNITS = (4, 8, 4)


def shufflenet(groups=3, scale=1.0, train_batch=32, test_batch=50, crop=224, classes=1000):
    """ShuffleNet v1 (Zhang et al. 2018, "ShuffleNet: An Extremely Efficient Convolutional Neural
    Network for Mobile Devices"): not in the reference.  ``conv1`` 3x3 / 2 to 24 channels and a 3x3 / 2
    max ``pool1``, then three stages of 4 / 8 / 4 units at SHUFFLENET_WIDTHS[groups] channels.  Unit
    ``resxN``: ``_conv1`` grouped 1x1 to a quarter of the stage width (ungrouped in the very first
    unit, whose input has 24 channels) with ReLU, ``shuffleN`` (ShuffleChannel), ``_conv2`` depthwise
    3x3 carrying the unit's stride, ``_conv3`` grouped 1x1 (csrc/kernels/conv_gpw.hip for both 1x1
    layers), then at stride 1 ``_elewise``, an Eltwise SUM with the unit's input, and at stride 2 (a
    stage's first unit) ``_concat`` with ``_match_conv``, a 3x3 / 2 average pooling of the input, where
    ``_conv3`` makes width - input channels; ReLU after either.  The pooling's pad (0 or 1) is the one
    at which Caffe's ceil-mode output size equals the depthwise layer's.  Global average ``pool_ave``
    (any crop) and the InnerProduct ``fc1000`` with bias.  Every conv is bias-free with in-place
    BatchNorm -> Scale [-> ReLU].  1 865 728 learnable elements besides the BatchNorm statistics at
    groups = 3, scale = 1, 1000 classes.  ``scale`` is the paper's width multiplier of the stages:
    scaled widths are rounded to multiples of 16 x groups, so that the channels per group of every
    grouped 1x1 stay multiples of 4 (what the kernels take; at scale 1 that holds for groups 1, 3, 8)."""
    def width(n):
        q = 16 * groups
        return n if scale == 1.0 else max(q, int(n * scale / q + 0.5) * q)

    def block(name, bottom, k, n, **kw):
        return _conv_bn(L, name, None, bottom, k, n, names=(name + "_bn", name + "_scale", name + "_relu"), **kw)

    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x, c = block("conv1", "data", 3, 24, stride=2, pad=1), 24
    L.append(_pool("pool1", x, 3, 2))
    x, h = "pool1", PoolSpec(1, (crop - 1) // 2 + 1, 1, 1, 3, 1, 2, 1).P
    unit = 0
    for stage, reps in enumerate(SHUFFLENET_UNITS):
        n = width(SHUFFLENET_WIDTHS[groups][stage])
        for r in range(reps):
            unit += 1
            tag, first = f"resx{unit}", r == 0
            y = block(tag + "_conv1", x, 1, n // 4, group=1 if unit == 1 else groups)
            L.append(ShuffleChannelLayer(f"shuffle{unit}", [y], groups))
            y = block(tag + "_conv2", f"shuffle{unit}", 3, n // 4, stride=2 if first else 1, pad=1, group=n // 4,
                      relu=False)
            y = block(tag + "_conv3", y, 1, n - c if first else n, group=groups, relu=False)
            if first:
                h2 = (h - 1) // 2 + 1  # the depthwise 3x3 / 2 with pad 1
                pad = next(p for p in (0, 1) if PoolSpec(1, h, 1, 1, 3, 1, 2, 1, p, 0).P == h2)
                L += [_pool(tag + "_match_conv", x, 3, 2, ave=True, pad=pad),
                      ConcatLayer(tag + "_concat", [tag + "_match_conv", y])]
                x, h = tag + "_concat", h2
            else:
                L.append(EltwiseLayer(tag + "_elewise", [x, y], "SUM"))
                x = tag + "_elewise"
            L.append(_relu(x + "_relu", x))
            c = n
    L += [PoolingLayer("pool_ave", [x], Pooling.Ave, global_pooling=True),
          _ip(f"fc{classes}", "pool_ave", classes, MSRA, _c(0.0)), *_head(f"fc{classes}", top5=True)]
    return NetParam(f"ShuffleNet-{scale:g}x-g{groups}", *L)


def _resnext_block(L, tag, bottom, width, cardinality, stride, project):
    """res{tag}: 1x1 -> grouped 3x3 (stride, ``cardinality`` groups: csrc/kernels/conv_grouped.hip)
    -> 1x1 (x2), summed with the input or its projection."""
    short = bottom
    if project:
        short = _conv_bn(L, f"res{tag}_branch1", f"{tag}_branch1", bottom, 1, 2 * width, stride=stride, relu=False)
    x = _conv_bn(L, f"res{tag}_branch2a", f"{tag}_branch2a", bottom, 1, width)
    x = _conv_bn(L, f"res{tag}_branch2b", f"{tag}_branch2b", x, 3, width, stride=stride, pad=1, group=cardinality)
    x = _conv_bn(L, f"res{tag}_branch2c", f"{tag}_branch2c", x, 1, 2 * width, relu=False)
    L += [EltwiseLayer(f"res{tag}", [short, x], "SUM"), _relu(f"res{tag}_relu", f"res{tag}")]
    return f"res{tag}"


def resnext(reps=(3, 4, 6, 3), cardinality=32, width=4, train_batch=32, test_batch=50, crop=224, classes=1000):
    """ResNeXt (Xie et al. 2017, "Aggregated Residual Transformations") in ResNet-50's layout and
    layer names: not in the reference.  Stage ``s`` (2..5) has ``reps[s - 2]`` bottlenecks of
    1x1 to D = cardinality * width * 2^(s - 2), a 3x3 with ``cardinality`` groups D -> D that
    carries the stage's stride, and 1x1 to 2 D; projection shortcuts where the shape changes.
    The defaults are ResNeXt-50 32x4d: 25 028 904 learnable elements besides the BatchNorm
    statistics."""
    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x = _conv_bn(L, "conv1", "_conv1", "data", 7, 64, stride=2, pad=3)
    L.append(_pool("pool1", x, 3, 2))
    x = "pool1"
    for stage, n in enumerate(reps, 2):
        d = cardinality * width * 2 ** (stage - 2)
        for r in range(n):
            x = _resnext_block(L, f"{stage}{chr(ord('a') + r)}", x, d, cardinality,
                               2 if (r == 0 and stage > 2) else 1, r == 0)
    L += [PoolingLayer("pool5", [x], Pooling.Ave, global_pooling=True),
          _ip(f"fc{classes}", "pool5", classes, MSRA, _c(0.0)), *_head(f"fc{classes}", top5=True)]
    return NetParam("ResNeXt", *L)


def resnext50(train_batch=32, test_batch=50, crop=224, classes=1000):
    """ResNeXt-50 32x4d: :func:`resnext` at its defaults."""
    return resnext(train_batch=train_batch, test_batch=test_batch, crop=crop, classes=classes)


def _se_block(L, tag, bottom, width, stride, project, reduction):
    """res{tag}: ResNet-50's bottleneck with a squeeze-and-excitation tail after scale{tag}_branch2c —
    global average pool, 1x1 down (ReLU), 1x1 up, Sigmoid — whose gate scales the block output
    inside the shortcut sum (Axpy: csrc/kernels/se.hip)."""
    short = bottom
    if project:
        short = _conv_bn(L, f"res{tag}_branch1", f"{tag}_branch1", bottom, 1, 4 * width, stride=stride, relu=False)
    x = _conv_bn(L, f"res{tag}_branch2a", f"{tag}_branch2a", bottom, 1, width, stride=stride)
    x = _conv_bn(L, f"res{tag}_branch2b", f"{tag}_branch2b", x, 3, width, pad=1)
    x = _conv_bn(L, f"res{tag}_branch2c", f"{tag}_branch2c", x, 1, 4 * width, relu=False)
    se = f"res{tag}_se"
    L += [PoolingLayer(se + "_pool", [x], Pooling.Ave, global_pooling=True),
          _conv(se + "_down", se + "_pool", 1, 4 * width // reduction, wf=MSRA, bf=_c(0.0)),
          _relu(se + "_down_relu", se + "_down"),
          _conv(se + "_up", se + "_down", 1, 4 * width, wf=MSRA, bf=_c(0.0)),
          SigmoidLayer(se + "_gate", [se + "_up"]),
          AxpyLayer(f"res{tag}", [se + "_gate", x, short]), _relu(f"res{tag}_relu", f"res{tag}")]
    return f"res{tag}"


def se_resnet(reps=(3, 4, 6, 3), reduction=16, train_batch=32, test_batch=50, crop=224, classes=1000):
    """SE-ResNet (Hu et al. 2018, "Squeeze-and-Excitation Networks"): not in the reference.
    ResNet-50's stem, bottlenecks and layer names with a squeeze-and-excitation tail per block:
    ``res{tag}_se_pool`` (global average), ``_se_down`` (1x1 convolution with bias to
    4 width / ``reduction``) with the in-place ``_se_down_relu``, ``_se_up`` (1x1 back to 4 width),
    ``_se_gate`` (Sigmoid), and ``res{tag}`` as an ``Axpy [gate, res{tag}_branch2c, shortcut]`` in
    place of the Eltwise SUM.  The block structure follows the public SENet Caffe release (the two
    SE products as 1x1 convolutions with bias, the Axpy tail); the names of the SE layers are this
    project's own — the release's prototxt was not at hand to compare, so a public .caffemodel
    will need its SE layers renamed.  At the defaults (SE-ResNet-50) 28 088 024 learnable elements
    besides the BatchNorm statistics: ResNet-50's 25 557 032 plus 2 530 992 in the sixteen SE pairs."""
    L = list(data_layers(train_batch, test_batch, 3, crop, crop))
    x = _conv_bn(L, "conv1", "_conv1", "data", 7, 64, stride=2, pad=3)
    L.append(_pool("pool1", x, 3, 2))
    x = "pool1"
    for stage, n in enumerate(reps, 2):
        width = 64 * 2 ** (stage - 2)
        for r in range(n):
            x = _se_block(L, f"{stage}{chr(ord('a') + r)}", x, width, 2 if (r == 0 and stage > 2) else 1, r == 0,
                          reduction)
    L += [PoolingLayer("pool5", [x], Pooling.Ave, global_pooling=True),
          _ip(f"fc{classes}", "pool5", classes, MSRA, _c(0.0)), *_head(f"fc{classes}", top5=True)]
    return NetParam("SE-ResNet", *L)


def se_resnet50(train_batch=32, test_batch=50, crop=224, classes=1000):
    """SE-ResNet-50: :func:`se_resnet` at its defaults."""
    return se_resnet(train_batch=train_batch, test_batch=test_batch, crop=crop, classes=classes)


# --- solvers ------------------------------------------------------------------------------

def _solver(net, **kw):
    s = proto.SolverParameter()
    s.net_param.CopyFrom(net)
    for k, v in kw.items():
        if isinstance(v, list):
            getattr(s, k).extend(v)
        else:
            setattr(s, k, v)
    return s


def lenet_solver(net=None):
    return _solver(net or lenet(), test_iter=[100], test_interval=500, base_lr=0.01, momentum=0.9,
                   weight_decay=5e-4, lr_policy="inv", gamma=1e-4, power=0.75, display=100, max_iter=10000)


def cifar10_quick_solver(net=None):
    return _solver(net or cifar10_quick(), test_iter=[100], test_interval=500, base_lr=0.001, momentum=0.9,
                   weight_decay=0.004, lr_policy="fixed", display=100, max_iter=4000)


def cifar10_full_solver(net=None):
    return _solver(net or cifar10_full(), test_iter=[100], test_interval=1000, base_lr=0.001, momentum=0.9,
                   weight_decay=0.004, lr_policy="fixed", display=200, max_iter=60000)


def caffenet_solver(net=None):
    return _solver(net or caffenet(), test_iter=[1000], test_interval=1000, base_lr=0.01, lr_policy="step",
                   gamma=0.1, stepsize=100000, display=20, max_iter=450000, momentum=0.9, weight_decay=5e-4)


def alexnet_solver(net=None):
    return caffenet_solver(net or alexnet())


def googlenet_solver(net=None):
    return _solver(net or googlenet(), test_iter=[1000], test_interval=4000, test_initialization=False, display=40,
                   average_loss=40, base_lr=0.01, lr_policy="step", stepsize=320000, gamma=0.96,
                   max_iter=10000000, momentum=0.9, weight_decay=2e-4)


def vgg16_solver(net=None):
    return _solver(net or vgg16(), test_iter=[1000], test_interval=10000, base_lr=0.01, lr_policy="step",
                   gamma=0.1, stepsize=100000, display=20, max_iter=370000, momentum=0.9, weight_decay=5e-4)


def resnet50_solver(net=None):
    return _solver(net or resnet50(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="step",
                   gamma=0.1, stepsize=150000, display=20, max_iter=600000, momentum=0.9, weight_decay=1e-4)


def resnet_cifar_solver(net=None):
    return _solver(net or resnet_cifar(), test_iter=[100], test_interval=1000, base_lr=0.1, lr_policy="multistep",
                   gamma=0.1, stepvalue=[32000, 48000], display=100, max_iter=64000, momentum=0.9, weight_decay=1e-4)


def mobilenet_solver(net=None):
    return _solver(net or mobilenet(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="poly", power=1.0,
                   display=20, max_iter=500000, momentum=0.9, weight_decay=4e-5)


def mnasnet_solver(net=None):  # MobileNet's schedule (the paper trains with RMSProp)
    return _solver(net or mnasnet(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="poly", power=1.0,
                   display=20, max_iter=500000, momentum=0.9, weight_decay=4e-5)


def shufflenet_solver(net=None):  # the paper's linear decay, as MobileNet's schedule here
    return _solver(net or shufflenet(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="poly", power=1.0,
                   display=20, max_iter=500000, momentum=0.9, weight_decay=4e-5)


def fcn8s_solver(net=None):  # the public voc-fcn8s solver: fixed rate on the unnormalised loss, high momentum
    return _solver(net or fcn8s(), test_iter=[736], test_interval=999999999, base_lr=1e-14, lr_policy="fixed",
                   display=20, max_iter=100000, momentum=0.99, weight_decay=5e-4)


def fast_rcnn_solver(net=None):  # the public Fast R-CNN solvers
    return _solver(net or fast_rcnn(), base_lr=0.001, lr_policy="step", gamma=0.1, stepsize=30000, display=20,
                   average_loss=100, max_iter=40000, momentum=0.9, weight_decay=5e-4)


def faster_rcnn_solver(net=None):  # the public stage-1 RPN solver of the alternating optimisation
    return _solver(net or faster_rcnn(), base_lr=0.001, lr_policy="step", gamma=0.1, stepsize=60000, display=20,
                   average_loss=100, max_iter=80000, momentum=0.9, weight_decay=5e-4)


def lrcn_solver(net=None):  # upstream's lstm_solver_RGB.prototxt
    return _solver(net or lrcn(), base_lr=0.001, lr_policy="step", gamma=0.1, stepsize=10000, display=20,
                   max_iter=30000, momentum=0.9, weight_decay=0.005, clip_gradients=5.0)


def resnext50_solver(net=None):  # ResNet-50's schedule
    return _solver(net or resnext50(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="step",
                   gamma=0.1, stepsize=150000, display=20, max_iter=600000, momentum=0.9, weight_decay=1e-4)


def se_resnet50_solver(net=None):  # ResNet-50's schedule
    return _solver(net or se_resnet50(), test_iter=[1000], test_interval=5000, base_lr=0.1, lr_policy="step",
                   gamma=0.1, stepsize=150000, display=20, max_iter=600000, momentum=0.9, weight_decay=1e-4)


MODELS = {
    "lenet": (lenet, lenet_solver), "cifar10_quick": (cifar10_quick, cifar10_quick_solver),
    "cifar10_full": (cifar10_full, cifar10_full_solver), "caffenet": (caffenet, caffenet_solver),
    "alexnet": (alexnet, alexnet_solver), "googlenet": (googlenet, googlenet_solver),
    "vgg16": (vgg16, vgg16_solver), "resnet50": (resnet50, resnet50_solver),
    "resnet_cifar": (resnet_cifar, resnet_cifar_solver), "mobilenet": (mobilenet, mobilenet_solver),
    "resnext50": (resnext50, resnext50_solver), "se_resnet50": (se_resnet50, se_resnet50_solver),
    "mnasnet": (mnasnet, mnasnet_solver), "shufflenet": (shufflenet, shufflenet_solver),
    "fcn8s": (fcn8s, fcn8s_solver), "fast_rcnn": (fast_rcnn, fast_rcnn_solver),
    "faster_rcnn": (faster_rcnn, faster_rcnn_solver), "lrcn": (lrcn, lrcn_solver),
}


def build(name: str, **kw):
    return MODELS[name][0](**kw)


def solver_for(name: str, **net_kw):
    net_fn, solver_fn = MODELS[name]
    return solver_fn(net_fn(**net_kw))
