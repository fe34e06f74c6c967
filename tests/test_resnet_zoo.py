"""The ResNet zoo entries on the CPU engine: the ResNet-50 parameter count, both phases of
both nets, one training step of the smallest CIFAR ResNet, and .caffemodel round trips of a
BatchNorm / Scale / Bias net through the Python and the native (libsn_core) readers."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from sparknet_amd import models, proto
from sparknet_amd.core.layer import layer_types
from sparknet_amd.core.net import Net
from sparknet_amd.core.solver import Solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net(param, phase, allocate=True):
    return Net(param, phase=phase, device="cpu", dtype=torch.float32, allocate=allocate)


def _learnable(net):
    return sum(p.count for layer in net.layers if layer.type_name != "BatchNorm" for p in layer.params)


def test_registry_has_scale_and_bias():
    assert {"Scale", "Bias", "BatchNorm", "Eltwise"} <= set(layer_types())
    assert {"resnet50", "resnet_cifar"} <= set(models.MODELS)


def test_resnet50_layout_and_parameter_count():
    param = models.resnet50()
    train = _net(param, proto.TRAIN, allocate=False)
    assert _learnable(train) == 25557032
    kinds = [layer.type_name for layer in train.layers]
    assert kinds.count("Convolution") == 53 and kinds.count("BatchNorm") == 53 and kinds.count("Scale") == 53
    assert kinds.count("Eltwise") == 16 and kinds.count("InnerProduct") == 1
    assert train.blob_by_name("conv1").shape == (32, 64, 112, 112)
    assert train.blob_by_name("pool1").shape == (32, 64, 56, 56)
    assert train.blob_by_name("res3a").shape == (32, 512, 28, 28)
    assert train.blob_by_name("res5c").shape == (32, 2048, 7, 7)
    assert train.blob_by_name("pool5").shape[:2] == (32, 2048)
    for layer in train.layers:
        if layer.type_name == "Convolution":
            assert len(layer.params) == 1, layer.name  # bias-free
        if layer.type_name == "BatchNorm":
            assert [p.lr_mult for p in layer.params] == [0.0, 0.0, 0.0] and not layer.use_global
        if layer.type_name == "Scale":
            li = train.layer_names.index(layer.name)
            assert len(layer.params) == 2 and train.bottom_ids[li] == train.top_ids[li]
    test = _net(param, proto.TEST, allocate=False)
    assert _learnable(test) == 25557032
    assert all(layer.use_global for layer in test.layers if layer.type_name == "BatchNorm")
    assert test.blob_by_name("fc1000").shape == (50, 1000)
    s = models.solver_for("resnet50", train_batch=2, test_batch=2, crop=64, classes=10)
    assert s.net_param.layer[0].java_data_param.shape.dim[0] == 2 and s.base_lr > 0


def test_resnet_cifar_builds_both_phases():
    for n, depth_convs in ((1, 9), (3, 21)):
        param = models.resnet_cifar(n=n, train_batch=4, test_batch=2)
        train, test = _net(param, proto.TRAIN), _net(param, proto.TEST)
        assert [l.type_name for l in train.layers].count("Convolution") == depth_convs  # 6n + 1 plus 2 projections
        assert train.blob_by_name("fc").shape == (4, 10) and test.blob_by_name("fc").shape == (2, 10)
        assert _learnable(train) == _learnable(test)


def test_resnet_cifar_cpu_training_step():
    sp = models.solver_for("resnet_cifar", n=1, train_batch=4, test_batch=4)
    sp.base_lr = 0.05
    solver = Solver(sp, device=torch.device("cpu"), build_test_nets=False)
    net = solver.net
    g = torch.Generator().manual_seed(0)
    net.blob_by_name("data").set_nchw(torch.randn(4, 3, 32, 32, generator=g))
    net.blob_by_name("label").data.copy_(torch.randint(0, 10, (4, 1), generator=g).float())
    before = net.flat_data.clone()
    loss = float(solver.iteration())
    assert loss == loss and 0 < loss < 50
    for layer in net.layers:
        for p in layer.params:
            changed = not torch.equal(net.flat_data[p.offset:p.offset + p.count], before[p.offset:p.offset + p.count])
            assert changed, (layer.name, p.name)  # BatchNorm statistics move too (forward update)


BN_NET = """
  name: "bn_scale_bias"
  layer { name: "data" type: "JavaData" top: "data" java_data_param { shape { dim: 4 dim: 3 dim: 8 dim: 8 } } }
  layer { name: "label" type: "JavaData" top: "label" java_data_param { shape { dim: 4 dim: 1 } } }
  layer { name: "conv1" type: "Convolution" bottom: "data" top: "conv1"
    convolution_param { num_output: 6 kernel_size: 3 bias_term: false weight_filler { type: "xavier" } } }
  layer { name: "bn1" type: "BatchNorm" bottom: "conv1" top: "conv1" }
  layer { name: "scale1" type: "Scale" bottom: "conv1" top: "conv1"
    scale_param { bias_term: true filler { type: "uniform" min: 0.5 max: 1.5 } } }
  layer { name: "relu1" type: "ReLU" bottom: "conv1" top: "conv1" }
  layer { name: "bias1" type: "Bias" bottom: "conv1" top: "b1" bias_param { filler { type: "gaussian" std: 0.1 } } }
  layer { name: "ip1" type: "InnerProduct" bottom: "b1" top: "ip1"
    inner_product_param { num_output: 3 weight_filler { type: "xavier" } } }
  layer { name: "loss" type: "SoftmaxWithLoss" bottom: "ip1" bottom: "label" top: "loss" }
"""


def _trained_bn_net(seed):
    net = Net(proto.parse_prototxt(BN_NET), phase=proto.TRAIN, seed=seed)
    g = torch.Generator().manual_seed(seed)
    net.blob_by_name("data").set_nchw(torch.randn(4, 3, 8, 8, generator=g))
    net.forward()  # moves the BatchNorm statistics off zero
    return net


def test_caffemodel_python_round_trip(tmp_path):
    a, b = _trained_bn_net(1), _trained_bn_net(2)
    assert not torch.equal(a.flat_data, b.flat_data)
    path = str(tmp_path / "bn.caffemodel")
    proto.write_binary(path, a.to_proto())
    saved = {l.name: l for l in proto.read_net(path).layer}
    assert [list(bp.shape.dim) for bp in saved["scale1"].blobs] == [[6], [6]]  # [scale, bias]
    assert [list(bp.shape.dim) for bp in saved["bn1"].blobs] == [[6], [6], [1]]
    assert [list(bp.shape.dim) for bp in saved["bias1"].blobs] == [[6]]
    b.copy_trained_layers_from(path)
    assert torch.equal(a.flat_data, b.flat_data)


def test_caffemodel_native_round_trip(tmp_path, monkeypatch):
    """The Python writer's file loads through the native reader and the native writer's through
    the Python reader, blob for blob."""
    from sparknet_amd import build_native
    core = build_native.build().get("core")
    if core is None:
        pytest.skip("libsn_core is not built")
    solver_txt = ('base_lr: 0.05 lr_policy: "fixed" momentum: 0.9 max_iter: 10 test_iter: 1 test_interval: 100000 '
                  'test_initialization: false net_param {' + BN_NET + '}')
    sp = tmp_path / "solver.prototxt"
    sp.write_text(solver_txt)
    lib = C.CDLL(core)
    lib.sn_create_state.restype = C.c_void_p
    lib.sn_last_error.restype = C.c_char_p
    lib.sn_num_params.restype = C.c_longlong
    st = C.c_void_p(lib.sn_create_state())
    buf, n = C.c_char_p(), C.c_int()
    assert lib.sn_parse_solver_prototxt(str(sp).encode(), C.byref(buf), C.byref(n)) == 0
    assert lib.sn_set_device(st, -1) == 0
    assert lib.sn_load_solver_from_protobuf(st, buf, n) == 0, lib.sn_last_error()
    nparam = lib.sn_num_params(st)

    def weights():
        out = (C.c_float * nparam)()
        assert lib.sn_get_weights(st, out, C.c_longlong(nparam)) == 0
        return np.frombuffer(out, dtype=np.float32).copy()

    src = _trained_bn_net(5)
    py = str(tmp_path / "python.caffemodel")
    proto.write_binary(py, src.to_proto())
    weights()  # builds the weights plan
    monkeypatch.setenv("SN_NATIVE_STEP", "1")
    assert lib.sn_load_weights_from_file(st, py.encode()) == 0, lib.sn_last_error()
    np.testing.assert_array_equal(weights(), src.flat_data.numpy()[:nparam])
    nat = str(tmp_path / "native.caffemodel")
    assert lib.sn_save_weights_to_file(st, nat.encode()) == 0, lib.sn_last_error()
    a, b = proto.read_net(nat), proto.read_net(py)
    blobs_b = {l.name: l.blobs for l in b.layer}
    for la in a.layer:
        assert len(la.blobs) == len(blobs_b[la.name]), la.name
        for x, y in zip(la.blobs, blobs_b[la.name]):
            assert list(x.shape.dim) == list(y.shape.dim)
            np.testing.assert_array_equal(np.asarray(x.data, np.float32), np.asarray(y.data, np.float32))
    dst = _trained_bn_net(6)
    dst.copy_trained_layers_from(nat)
    assert torch.equal(dst.flat_data, src.flat_data)
