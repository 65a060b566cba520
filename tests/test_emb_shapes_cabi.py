"""The shape rules the embedder's training path shares (csrc/emb_host.h), seen through the C-ABI: the forward tail
(dsmil_trunk32_tail) and the norm backward (dsmil_norm_bwd*) take the same channel counts up to the backward's own limit of 2048,
so a block whose eligibility is asked of the norm backward is taken by the tail too; and the three conv families (trunk32,
conv backward, trunk16) agree on a conv's output map wherever more than one accepts the shape.  Pins behaviour: nothing here
launches (an accepted shape is answered DSMIL_E_ALIGN through a mis-aligned ``out``).  CPU only."""
import ctypes
import itertools

import pytest

import dsmil  # noqa: F401  (registers the dsmil_wsi_amd package)
import dsmil_wsi_amd._native as nat
from dsmil_wsi_amd import ops

E_UNSUPPORTED, E_ALIGN = -2, -5
BIG = 1 << 30


def chan_rule(C):
    """C / 4 channel groups divide the 256 threads of a workgroup or are a multiple of them."""
    return C % 4 == 0 and (256 % (C // 4) == 0 if C // 4 < 256 else (C // 4) % 256 == 0)


@pytest.fixture(scope="module")
def ptrs():
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    p = ctypes.c_void_p
    return buf, [p(a + 256 * i) for i in range(6)], p(a + 4)       # (keeps buf alive), aligned pointers, a 4-byte aligned one


def test_the_tail_takes_exactly_the_channel_rule(ptrs):
    _, (P, Q, R, S, _, _), odd4 = ptrs
    tail = nat.lib().dsmil_trunk32_tail
    took = []
    for C in range(1, 4201):
        rc = tail(0, P, Q, R, S, None, None, odd4, 1, 1, C, 0, None)
        assert rc in (E_ALIGN, E_UNSUPPORTED), (C, rc)
        assert (rc == E_ALIGN) == chan_rule(C), (C, rc)
        if rc == E_ALIGN:
            took.append(C)
    assert took == [4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 3072, 4096]


def test_every_width_the_norm_backward_takes_the_tail_takes():
    size = nat.lib().dsmil_norm_bwd_workspace_bytes
    for kind in ops.NORM_BWD_KINDS.values():
        for C in range(1, 4201):
            assert (size(kind, 1, 1, C) > 0) == (chan_rule(C) and C <= 2048), (kind, C)


def _trunk16_out(Cin, Cout, ks, stride, pad, H, W, ptrs):
    """(Ho, Wo) as the caller of dsmil_trunk16_conv must size ``out16`` where the entry accepts the shape (answered by
    DSMIL_E_ALIGN: out16 mis-aligned), else None.  The entry returns no map; its documented one is positions(B, Ho, Wo)."""
    _, (P, Q, _, _, _, W256), odd4 = ptrs
    rc = nat.lib().dsmil_trunk16_conv(P, Q, odd4, 1, H, W, Cin, Cout, ks, stride, pad, 1, W256, BIG, None)
    assert rc in (E_ALIGN, E_UNSUPPORTED), rc
    return ops._conv_out(H, W, ks, stride, pad) if rc == E_ALIGN else None


def test_the_conv_families_agree_on_the_output_map(ptrs):
    accepted = {"trunk32": 0, "weight": 0, "data": 0, "trunk16": 0}
    several = 0
    for ks, stride, pad, H, W in itertools.product((1, 2, 3, 5, 7), (1, 2, 3), (0, 1, 2, 3), (1, 2, 5, 7), (1, 2, 5, 7)):
        for Cin, Cout in ((64, 64), (64, 128), (3, 64)):
            maps = {}
            try:
                p = ops.trunk32_conv_plan(Cin, Cout, ks, stride, pad, 1, H, W)
                # a Winograd plan reports the map it tiles, which is the input's: 3x3 / stride 1 / pad 1 keeps the size
                maps["trunk32"] = (p["Ho"], p["Wo"])
            except NotImplementedError:
                pass
            for which in ("weight", "data"):
                try:
                    p = ops.conv_backward_plan(Cin, Cout, ks, stride, pad, 1, H, W, which)
                    maps[which] = (p["Ho"], p["Wo"])
                except NotImplementedError:
                    pass
            t16 = _trunk16_out(Cin, Cout, ks, stride, pad, H, W, ptrs)
            if t16 is not None:
                maps["trunk16"] = t16
            for k in maps:
                accepted[k] += 1
            # a size query that answers is the same acceptance as its plan entry
            assert ops.trunk32_conv_supported(Cin, Cout, ks, stride, pad, 1, H, W) == ("trunk32" in maps)
            assert ops.conv_backward_supported(Cin, Cout, ks, stride, pad, 1, H, W, "weight") == ("weight" in maps)
            assert ops.conv_backward_supported(Cin, Cout, ks, stride, pad, 1, H, W, "data") == ("data" in maps)
            if maps:
                want = ops._conv_out(H, W, ks, stride, pad)
                assert min(want) >= 1, (ks, stride, pad, H, W, maps)             # no family takes a conv without an output pixel
                assert all(m == want for m in maps.values()), (Cin, Cout, ks, stride, pad, H, W, maps)
                several += len(maps) > 1
    assert all(n > 0 for n in accepted.values()), accepted
    assert several > 100, several
