"""CPU-only, no convolution or pooling kernel: the GRUNet module's host side -- the layer table against the reference's stored key list, the seeded
weights, the MAC count DESIGN.md states, the packing of a transposed layer (the packing kernel alone, under the SIMT emulator) against NumPy,
and the errors that are raised before anything is launched."""
import os
import re

import numpy as np
import pytest
import torch

import dprox as dp
import grunet_cases as gc
from conftest import ROOT
from dprox.proxfn.pnp.denoisers import grunet_layer_table, grunet_macs_per_voxel


def test_state_dict_keys_are_the_reference_s():
    net = dp.GRUnet(in_ch=2)
    sd = net.state_dict()
    assert list(sd) == [str(k) for k in gc.golden()["keys"]]
    assert len(sd) == 35 and sum(v.numel() for v in sd.values()) == 14278451
    assert [k for k in sd if k.endswith("bias")] == ["Conv.conv.deconv.bias"] and tuple(sd["Conv.conv.deconv.bias"].shape) == (3,)
    assert tuple(sd["Up_conv5.conv1.conv.deconv.weight"].shape) == (256, 256, 3, 3, 3) and tuple(sd["Conv1.conv.conv.weight"].shape) == (48, 2, 3, 3, 3)
    assert tuple(dp.GRUnet(in_ch=1).state_dict()["Conv1.conv.conv.weight"].shape) == (48, 1, 3, 3, 3)


def test_checkpoint_forms_load(tmp_path):
    net = dp.GRUnet(in_ch=2)
    w = gc.grunet_weights(3, [(k, tuple(v.shape)) for k, v in net.state_dict().items()])
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    path = os.path.join(str(tmp_path), "unet_qrnn3d.pth")
    torch.save({"net": sd, "epoch": 7}, path)
    den = dp.GRUNetDenoiser(path)
    for k, v in den.model.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert all(not p.requires_grad for p in den.parameters())
    with pytest.raises(RuntimeError, match="Missing|Unexpected"):
        dp.GRUnet(in_ch=2).load_reference_state_dict({**sd, "Conv.bn.weight": torch.zeros(1)})


def test_grunet_weights_are_reproducible():
    shapes = [(k, tuple(v.shape)) for k, v in dp.GRUnet(in_ch=2).state_dict().items()][:6]
    a, b, c = gc.grunet_weights(5, shapes), gc.grunet_weights(5, shapes), gc.grunet_weights(6, shapes)
    for k, shape in shapes:
        assert a[k].dtype == np.float32 and a[k].shape == shape and np.array_equal(a[k], b[k]) and not np.array_equal(a[k], c[k])
        assert np.abs(a[k]).max() <= 1.0 / np.sqrt(shape[1] * 27) and np.abs(a[k]).max() > 0.9 / np.sqrt(shape[1] * 27)


def test_mac_count_of_design_md():
    """DESIGN.md's "GRUNet" section states the multiply-adds per full-resolution voxel: the number the module's layer table gives"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    m = re.search(r"([\d ]+) multiply-adds per full-resolution voxel", text[text.index("GRUNet"):])
    assert m, "DESIGN.md does not state the count"
    assert int(m.group(1).replace(" ", "")) == grunet_macs_per_voxel(2) == 382256
    per_level = {}
    for _, form, cin, hidden, direction, _, level in grunet_layer_table(2):
        per_level[level] = per_level.get(level, 0) + (1 if form == "k1" else 27) * cin * hidden * (3 if direction == "bi" else 2)
    assert per_level[0] == 2592 + 27648 + 42496 + 1296           # Conv1, Up2, Up_conv2, Conv


def test_packing_of_a_transposed_layer():
    """dpx_qrnn3d_pack on a ConvTranspose3d tensor [cin][cout][27]: flipped taps, swapped channel axes, [chunk][tap][plane][k-group][row][8]"""
    import emul_util
    be = emul_util.use_emulator()
    cin, cout = 24, 40                                            # two chunks (the second half empty), 64 rows of which 40 are used
    rng = np.random.RandomState(0)
    w = rng.randn(cin, cout, 3, 3, 3).astype(np.float32)
    b = rng.randn(cout).astype(np.float32)
    for mode, planes in ((3, 2), (6, 3)):
        blob = gc.pack_layer(be.lib(), w, b, 0, cin, cout, True, mode, "cpu").numpy()
        M32, chunks = 64, 2
        nw = chunks * 27 * planes * 2 * M32 * 8
        assert blob.size == nw * 2 + M32 * 4 == be.lib().query("dpx_qrnn3d_packed_bytes", 0, cin, cout, mode)
        wp = blob[:nw * 2].view(np.uint16).reshape(chunks, 27, planes, 2, M32, 8)
        conv = np.zeros((M32, chunks * 16, 27), np.float32)      # the equivalent Conv3d tensor [cout][cin][tap]
        conv[:cout, :cin] = w.reshape(cin, cout, 27)[:, :, ::-1].transpose(1, 0, 2)
        want = conv.reshape(M32, chunks, 2, 8, 27).transpose(1, 4, 2, 0, 3)          # [chunk][tap][k-group][row][8]
        if mode == 3:
            hi = want.astype(np.float16)
            lo = ((want - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
            parts = [hi.view(np.uint16), lo.view(np.uint16)]
        else:
            parts, rest = [], want.copy()
            for _ in range(3):
                t = (rest.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
                parts.append((t.view(np.uint32) >> 16).astype(np.uint16))
                rest = rest - t
        for p in range(planes):
            assert np.array_equal(wp[:, :, p], parts[p]), (mode, p)
        bias = blob[nw * 2:].view(np.float32)
        assert np.array_equal(bias[:cout], b) and not bias[cout:].any()
    with pytest.raises(be.DpxError, match="transposed"):
        gc.pack_layer(be.lib(), w, None, 1, cin, cout, True, 3, "cpu")


def test_errors_before_any_launch():
    den = dp.GRUNetDenoiser()
    s = torch.tensor(0.1)
    with torch.no_grad():
        with pytest.raises(ValueError, match="multiples of 16"):
            den.denoise(torch.zeros(1, 3, 24, 16), s)
        with pytest.raises(ValueError, match="4-D"):
            den.model(torch.zeros(3, 16, 16), s)
    with pytest.raises(NotImplementedError, match="forward-only"):
        den.denoise(torch.zeros(1, 3, 16, 16, requires_grad=True), s)
    with pytest.raises(NotImplementedError):
        dp.GRUnet(in_ch=2, bn=True)
    with pytest.raises(NotImplementedError):
        dp.GRUNetTVDenoiser("x.pth")
    with pytest.raises(NotImplementedError):
        dp.QRNN3DDenoiser("x.pth")
    with pytest.raises(NotImplementedError):
        dp.deep_prior(dp.Variable(), "qrnn3d")
    bad = dp.GRUNetDenoiser()
    bad.model.compute_mode = "f32"
    with pytest.raises(ValueError, match="compute_mode"), torch.no_grad():
        bad.denoise(torch.zeros(1, 3, 16, 16), s)
