"""The fp64 reference of tests/launch_ref.py against stock torch restatements of the layers (autograd through nn modules),
and the committed launch census against ops' fixed tables.  No GPU needed."""
import json
import os

import pytest
import torch
import torch.nn as nn

import launch_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
KH = {"k1": 1, "k3s1": 3, "k4s2": 4, "up": 3}


def stock_layer(layer, I, O):
    """The reference model's modules for the layer (model.py: conv1x1 / conv3x3 / downBlock conv / upBlock)."""
    if layer == "k1":
        return nn.Conv2d(I, O, 1, bias=False)
    if layer == "k3s1":
        return nn.Conv2d(I, O, 3, 1, 1, bias=False)
    if layer == "k4s2":
        return nn.Conv2d(I, O, 4, 2, 1, bias=False)
    return nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(I, O, 3, 1, 1, bias=False))


@pytest.mark.parametrize("layer", R.LAYERS)
@pytest.mark.parametrize("B,I,O,H", [(2, 5, 7, 8), (3, 4, 3, 4)])
def test_reference_matches_stock_autograd(layer, B, I, O, H):
    g = torch.Generator().manual_seed(11)
    m = stock_layer(layer, I, O).double()
    conv = m if isinstance(m, nn.Conv2d) else m[1]
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g, dtype=torch.float64))
    x = torch.randn(B, I, H, H, generator=g, dtype=torch.float64, requires_grad=True)
    y = m(x)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    w = conv.weight.detach()
    torch.testing.assert_close(R.fwd(layer, x.detach(), w), y.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.dgrad(layer, dy, w), x.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(R.wgrad(layer, x.detach(), dy, KH[layer]), conv.weight.grad, rtol=1e-12, atol=1e-12)
    if layer == "k1":     # nn.Linear weights (O, I) go through the same 1x1 operation
        torch.testing.assert_close(R.fwd(layer, x.detach(), w[:, :, 0, 0]), y.detach(), rtol=1e-12, atol=1e-12)


def test_class_bias_equals_broadcast_channels():
    """A spatially constant operand concatenated first (torch.cat((c_code, h), 1) then conv3x3) equals the conv of h plus
    the class-bias table indexed by border class; the table is that operand's conv on a 3 x 3 map, whose pixel (i, j) is
    the representative of class 3 i + j."""
    g = torch.Generator().manual_seed(3)
    B, Cc, Cx, N, H = 2, 4, 6, 5, 8
    c = torch.randn(B, Cc, generator=g, dtype=torch.float64)
    x = torch.randn(B, Cx, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(N, Cc + Cx, 3, 3, generator=g, dtype=torch.float64)
    full = nn.functional.conv2d(torch.cat((c.view(B, Cc, 1, 1).expand(B, Cc, H, H), x), 1), w, padding=1)
    table = nn.functional.conv2d(c.view(B, Cc, 1, 1).expand(B, Cc, 3, 3), w[:, :Cc], padding=1)
    table = table.reshape(B, N, 9).permute(0, 2, 1)
    got = R.add_class_bias(R.fwd("k3s1", x, w[:, Cc:]), table)
    torch.testing.assert_close(got, full, rtol=1e-12, atol=1e-12)
    cls = R.border_class(4, 4)
    assert cls.tolist() == [[0, 1, 1, 2], [3, 4, 4, 5], [3, 4, 4, 5], [6, 7, 7, 8]]


def test_group_stats():
    g = torch.Generator().manual_seed(4)
    y = torch.randn(6, 3, 2, 2, generator=g, dtype=torch.float64)
    s = R.group_stats(y, 3)
    for k in range(3):
        yk = y[2 * k:2 * k + 2].permute(1, 0, 2, 3).reshape(3, -1)
        torch.testing.assert_close(s[0, k], yk.sum(1))
        torch.testing.assert_close(s[1, k], (yk * yk).sum(1))
    torch.testing.assert_close(R.group_stats(y, 0), R.group_stats(y, 1))


def test_census_maps_to_layer_operations():
    """The committed census holds both workloads, and each entry maps to exactly one layer operation through ops' fixed
    tables; a weight's pack mode is the one that operation uses."""
    with open(os.path.join(HERE, "step_launches.json")) as fp:
        census = json.load(fp)
    assert sorted(census) == ["bf16_b48", "fp32_b24"]
    for mode, recs in census.items():
        assert recs, mode
        keys = [json.dumps(r, sort_keys=True) for r in recs]
        assert len(set(keys)) == len(keys), mode
        for rec in recs:
            op, layer = R.layer_op(rec)
            if rec["fn"].startswith("conv") and rec["w"]["oihw"] is not None:
                assert rec["w"]["mode"] == R.pack_mode(op, layer), rec
            if op == "wgrad":
                assert len(rec["grad_shape"]) == 2 or rec["grad_shape"][2] == KH[layer], rec
