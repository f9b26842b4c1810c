"""The packed weight buffer byte for byte (udf_mlp.hip: rowscale_kernel + pack_all_kernel).

Every kernel that reads the buffer is checked only through end-to-end tolerances; a wrong lo part, scale byte or PE slot could hide
under them.  Each case fills the buffer with 0xA5, re-packs it in place and compares the sha256 of the whole buffer with the digest
recorded here, so the bytes the packer leaves alone (alignment padding) are pinned as well.  The weights come from
synthetic.make_udf_state (numpy PCG64): they do not depend on the torch version."""
import hashlib

import pytest
import torch

import emap_amd
from emap_amd import synthetic
from conftest import NETS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PACK_NETS = {
    "d8w256L10": NETS["d8w256L10"],
    "d8w256L6": NETS["d8w256L6"],
    "d4w128L10": NETS["d4w128L10"],   # skip layer = last layer: has_rev = 0, no swm section
    "d8w256L0": (dict(d_in=3, d_out=1, d_hidden=256, n_layers=8, skip_in=(4,), multires=0, bias=0.5), 46, 0.02),
    "d8w128L10": (dict(d_in=3, d_out=1, d_hidden=128, n_layers=8, skip_in=(4,), multires=10, bias=0.5), 48, 0.02),   # transposed section at H = 128
}
PRECS = ["bf16", "bf16x3", "f16", "f16x3", "f16x3e", "f16x3m"]
CASES = [(n, p) for n in PACK_NETS for p in PRECS if p != "f16x3m" or PACK_NETS[n][0]["d_hidden"] == 256]   # f16x3m needs d_hidden = 256

# recorded on an MI355X from the packer as it stood before its fragment bodies were consolidated
DIGESTS = {
    ("d8w256L10", "bf16"): "3f5b33c4df0eb42435b9f1fd9c0b82bfca637794be1e73dec3e4f99286c369f8",
    ("d8w256L10", "bf16x3"): "4dd798968897b0ea8b1b715dd5ab302a3fbfd581e9281f504ebce036a351bd2d",
    ("d8w256L10", "f16"): "3d8623e4f6f528b013d7ced7f8bfb1d917e28cf3c194bb0f51f6f2a5c399cdd3",
    ("d8w256L10", "f16x3"): "d1e2c75b1a2069d7bae241c27c966f0ad013cbdf48ad83d26304cd386e044692",
    ("d8w256L10", "f16x3e"): "89f7d92f2a4a23fc427a123c8e8a6694cc9750036020189fd385be6b3c9dc9ba",
    ("d8w256L10", "f16x3m"): "30eb39a70b9872947cde6fad54e005e6885cdde25999a3fec68e8f82bb7e573e",
    ("d8w256L6", "bf16"): "f3d41b8155425ef6d9867025d50a06ea95ff1d4eb4585ce6d92fca97a0314aef",
    ("d8w256L6", "bf16x3"): "5bbc919cb8f5abc77ecf45d708e57818474eedfc60e98456757a64e110a9ef4a",
    ("d8w256L6", "f16"): "8f75790145aa50ec258992f1dc4e43f251db9fa72e96f0540172de41baf41245",
    ("d8w256L6", "f16x3"): "d71c202b53f0638626031944679d38678f359bd366c74fa9fe221deffd4613c9",
    ("d8w256L6", "f16x3e"): "b64b13c96bbd1973038d18b2f42d2c2e152909d9c32920e9b0ed45d2a58e85d9",
    ("d8w256L6", "f16x3m"): "981e9640708b6f7949d00f773e3138246e1afbc032f9459914a07421235971e7",
    ("d4w128L10", "bf16"): "e1365a796a6e1ed1694b7a8b00102c82e40c35ee39ef02c9ef59fb0efb9e5f88",
    ("d4w128L10", "bf16x3"): "9dbf407cc830f122fdb263644b6d86dc10693f56a7a15ea7ac7042434992b3b0",
    ("d4w128L10", "f16"): "39ae18125b4715fadd2ca686e0ff13761ccbf3c34eb3b73188b646c894370e69",
    ("d4w128L10", "f16x3"): "d59a35f77cafa02d300713539f91033e5260b74a969f715bfd1966f7e52fa1af",
    ("d4w128L10", "f16x3e"): "d59a35f77cafa02d300713539f91033e5260b74a969f715bfd1966f7e52fa1af",
    ("d8w256L0", "bf16"): "76aabc9cd28f6ced1ba62bbc58cd47a9fc8aa45c2253f710a15fd52da4037178",
    ("d8w256L0", "bf16x3"): "23e7505f350f3c020584640bd4462772bc5fb94419360cae42c16c97e01d8c34",
    ("d8w256L0", "f16"): "03e697f2d9aaec0e636cc8c562f54b56dce36173bcc4bdab7378096d64002eaa",
    ("d8w256L0", "f16x3"): "65d3a1436610d159933c77b78f2942a18709125ab49b3e5411c032f3367e0dc1",
    ("d8w256L0", "f16x3e"): "a179bbac6064523f59d9c772293f4787043ed3a88b84893bc4715e78223c349c",
    ("d8w256L0", "f16x3m"): "ad403a78b9fa04cd840c2ebc707e23c3c5bd823fe1c9fa35fdbda9e4d718fcad",
    ("d8w128L10", "bf16"): "f99edbe366e0119692dba65e809393bda651c57de83119574344c6e25a055083",
    ("d8w128L10", "bf16x3"): "699830478c56fc3ded53d8940bc0f21da2a465ab76b665583c898ff0df787b75",
    ("d8w128L10", "f16"): "ad0c26c5152e6551df8b499f5c6a0bafd3e8047f4098af9cbb3141b1d729509b",
    ("d8w128L10", "f16x3"): "8d44307c42908f9c6df576edfce2d8fe6a74a9e6aef057d2434eb86c08a16546",
    ("d8w128L10", "f16x3e"): "8d44307c42908f9c6df576edfce2d8fe6a74a9e6aef057d2434eb86c08a16546",
}


def packed_digest(name, prec):
    kw, seed, pert = PACK_NETS[name]
    net = emap_amd.UDFNetwork(scale=1.0, precision=prec, **kw)
    net.load_state_dict(synthetic.make_udf_state(seed=seed, pert=pert, **kw))
    net = net.to(DEV)
    buf = net.packed(prec)
    buf.fill_(0xA5)
    net.invalidate_packed()
    assert net.packed(prec).data_ptr() == buf.data_ptr()   # re-packed in place
    torch.cuda.synchronize()
    return hashlib.sha256(buf.cpu().numpy().tobytes()).hexdigest()


@pytest.mark.parametrize("name,prec", CASES)
def test_packed_bytes(name, prec):
    assert packed_digest(name, prec) == DIGESTS[(name, prec)]
