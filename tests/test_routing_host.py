"""Routing of fmri_igemm_ep, asked of the library itself through fmri_igemm_route: host code only, no GPU needed.
Besides the headline layers, one case per fall-through rule of csrc/api.hip's family selectors -- the statistics-row
planner's two decline policies, the kill switches and argument validation -- with the names the library gave before
the router was split into selectors."""
import os
import subprocess
import sys

import pytest

from fmri_hip import lib
from fmri_hip.ops import igemm_route as route, MODE_CONV, MODE_TCONV2, ACT_NONE

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _tconv_elems(ci, rows_pad):
    return max(g["w_off"] + rows_pad * g["kpad"] for g in (lib.tconv_class(5, 2, cy, cx, ci, rows_pad)
                                                            for cy in range(2) for cx in range(2)))


def conv(N, H, ci, co, **kw):
    return route(N, H, H, ci, H // 2, H // 2, co, co, 5, 2, 2, MODE_CONV, ACT_NONE, False, 1, 128, co * lib.kpad(25, ci),
                 **kw)


def tconv(N, H, ci, co, tile=128, **kw):
    return route(N, H, H, ci, 2 * H, 2 * H, co, co, 5, 2, 2, MODE_TCONV2, ACT_NONE, False, 1, tile,
                 _tconv_elems(ci, max(co, tile)), **kw)


def test_kernel_routing_of_the_headline_layers():
    """fmri_igemm_route -- the library's own statement of csrc/api.hip's routing, host code that needs no GPU (bench.py
    prices kernel families by it): the stride-2 layers of the B = 256 Stage-I step go to the 8-wave loader / compute kernels
    of round 3, the 32-channel and 64-channel-tile ones stay where they were, and a request for the BatchNorm-backward
    epilogue is never routed to a kernel without one."""
    from fmri_hip import lib
    from fmri_hip.ops import igemm_route as route, MODE_CONV, MODE_TCONV2, ACT_NONE, ACT_RELU

    def tconv_elems(ci, rows_pad):
        return max(g["w_off"] + rows_pad * g["kpad"] for g in (lib.tconv_class(5, 2, cy, cx, ci, rows_pad)
                                                                for cy in range(2) for cx in range(2)))
    conv = lambda N, H, ci, co, **kw: route(N, H, H, ci, H // 2, H // 2, co, co, 5, 2, 2, MODE_CONV, ACT_NONE, False, 1, 128,
                                            co * lib.kpad(25, ci), **kw)
    tconv = lambda N, H, ci, co, tile=128, **kw: route(N, H, H, ci, 2 * H, 2 * H, co, co, 5, 2, 2, MODE_TCONV2, ACT_NONE,
                                                       False, 1, tile, tconv_elems(ci, max(co, tile)), **kw)
    assert conv(768, 32, 128, 256) == "fmri::igemm_c5w_kernel<16,0>"     # discriminator.conv.2 forward
    assert conv(768, 32, 128, 256, stat_rows_cap=4096) == "fmri::igemm_c5w_kernel<16,1>"     # ... with BatchNorm statistics
    assert conv(768, 64, 32, 128).startswith("fmri::igemm_c5w_kernel<16")   # discriminator.conv.1 forward (one sub-chunk)
    assert conv(768, 16, 256, 256) == "fmri::igemm_c5w_kernel<8,0>"      # discriminator.conv.3 forward (8 x 8 outputs)
    assert tconv(1536, 16, 256, 128) == "fmri::igemm_tc5w_kernel<16,0,false>"    # discriminator.conv.2 data gradient
    assert tconv(1536, 8, 256, 256) == "fmri::igemm_tc5w_kernel<8,0,false>"      # discriminator.conv.3 data gradient
    assert tconv(256, 8, 256, 128) == "fmri::igemm_tc5w_kernel<8,0,true>"        # encoder.conv.2 data gradient: one class per block
    assert tconv(512, 16, 256, 128, stat_rows_cap=4096) == "fmri::igemm_tc5w_kernel<16,1,false>"   # decoder.conv.1 forward
    assert tconv(256, 16, 128, 64, 64).startswith("fmri::igemm_tc5_kernel<64")   # encoder.conv.1 data gradient
    assert tconv(512, 32, 128, 32, 32) == "fmri::igemm_tc32_kernel<false>"   # decoder.conv.2 forward
    assert tconv(1536, 32, 128, 32, 32, want_act_y=True) == "fmri::igemm_tc32_kernel<true>"   # discriminator.conv.1 dgrad + ReLU mask
    # the BatchNorm-backward epilogue exists in the narrower kernels only (advisor finding of round 3: the request must
    # decide, not the row capacity)
    assert conv(512, 32, 128, 256, stat_rows_cap=4096, want_bn_bwd=True).startswith("fmri::igemm_c5_kernel<16,2")
    assert conv(512, 32, 128, 256, stat_rows_cap=1, want_bn_bwd=True).startswith("fmri::igemm_c5_kernel<16,0")
    assert tconv(512, 16, 256, 128, stat_rows_cap=4096, want_bn_bwd=True).startswith("fmri::igemm_tc5_kernel<128")
    # small-channel stride-1 layers and the dense layers
    n = lambda N, ci, co, mode=MODE_CONV, act=ACT_NONE, bias=False: route(N, 64, 64, ci, 64, 64, co, min(co, 3) if co == 8 else co,
                                                                          5, 1, 2, mode, act, False, 1, 32, 32 * lib.kpad(25, ci),
                                                                          has_bias=bias)
    assert n(768, 8, 32, act=ACT_RELU, bias=True) == "fmri::igemm_narrow_kernel<8,2,false>"      # discriminator.conv.0
    assert n(512, 32, 8).startswith("fmri::igemm_narrow_kernel<32,1")                             # decoder.conv.3
    dense = route(256, 1, 1, 16384, 1, 1, 1024, 1024, 1, 1, 0, MODE_CONV, ACT_NONE, True, 8, 64, 1024 * 16384)
    assert dense == "fmri::igemm_kernel<128,64,2,2,true,true>", dense


def test_statistics_rows_that_do_not_fit():
    """The narrow forms write plain output when a group's rows exceed rows_cap; the wide forms leave the call to them."""
    assert conv(768, 32, 128, 256, stat_rows_cap=1) == "fmri::igemm_c5_kernel<16,0>"
    assert tconv(512, 16, 256, 128, stat_rows_cap=1) == "fmri::igemm_tc5_kernel<128,6,0>"


def test_statistics_groups_that_would_share_a_tile():
    """c5w / tc5w take four 8 x 8 images per tile: groups of two images go to the two-image-tile narrow forms."""
    assert conv(768, 16, 256, 256, stat_rows_cap=4096, stat_group_n=2) == "fmri::igemm_c5_kernel<8,1>"
    assert conv(768, 16, 256, 256, stat_rows_cap=4096, stat_group_n=4) == "fmri::igemm_c5w_kernel<8,1>"
    assert tconv(1536, 8, 256, 256, stat_rows_cap=4096, stat_group_n=2) == "fmri::igemm_tc5_kernel<128,4,1>"
    assert tconv(1536, 8, 256, 256, stat_rows_cap=4096, stat_group_n=4) == "fmri::igemm_tc5w_kernel<8,1,false>"


def test_bad_epilogue_arguments():
    for kw in (dict(want_affine=True, stat_rows_cap=4096),      # affine and statistics together
               dict(want_bn_bwd=True),                           # BatchNorm backward without statistics
               dict(stat_rows_cap=4096, stat_group_n=5)):        # groups that do not divide the batch
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            conv(768, 32, 128, 256, **kw)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):      # statistics of an fp32 output
        route(256, 1, 1, 16384, 1, 1, 1024, 1024, 1, 1, 0, MODE_CONV, ACT_NONE, True, 1, 64, 0, stat_rows_cap=4096)


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {pkg!r}]
from tests.test_routing_host import conv, tconv
print(conv(768, 32, 128, 256)); print(tconv(1536, 16, 256, 128))
"""


@pytest.mark.parametrize("env, conv_name, tconv_name", [
    (dict(FMRI_C5="off"), "fmri::igemm_kernel<256,256,2,4,false,true>", "fmri::igemm_tc5w_kernel<16,0,false>"),
    (dict(FMRI_C5W="off"), "fmri::igemm_c5_kernel<16,0>", "fmri::igemm_tc5w_kernel<16,0,false>"),
    (dict(FMRI_TC5W="off"), "fmri::igemm_c5w_kernel<16,0>", "fmri::igemm_tc5_kernel<128,6,0>"),
    (dict(FMRI_TC5="off"), "fmri::igemm_c5w_kernel<16,0>", "fmri::igemm_kernel<128,128,2,2,false,true>"),
    (dict(FMRI_C5W="on"), "fmri::igemm_c5w_kernel<16,0>", "fmri::igemm_tc5w_kernel<16,0,false>"),   # only "off"
])
def test_kill_switches(env, conv_name, tconv_name):
    """The switches are read once per process, so each setting runs in a child.  c5w sits inside the c5 switch and tc5w
    inside the tc5 switch."""
    code = _CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "thesis-fmri-reconstruction_amd"))
    out = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split() == [conv_name, tconv_name]
