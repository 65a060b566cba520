"""The fragment order of k_attend_f3's weights (csrc/agg_f2.h: f3_unit, f3_frag_map, f3_frag_slot), restated in numpy from the
header's formulas.  v_mfma_f32_16x16x32_f16: lane (m = lane & 15, g = lane >> 4) of a fragment holds the k-slots 8g .. 8g+7
of row m of a 16-unit block.  The kernel reads its fragments out of the image k_pack_agg_f2 writes for k_attend_f2, whose
order does not change.

* every (unit, k, plane) of W1 and of W2 sits in exactly one (chunk, unit block, plane, lane, element);
* the 16-byte slot f3_frag_slot names holds, by k_pack_agg_f2's own formula, exactly the eight (unit, k) of the fragment's
  lane, for W1 and for W2, and every slot of the image is taken once;
* W2's k order is the order in which the hidden cut of k_attend_f3 lays a row's hidden units into LDS, and the units a lane
  holds of an accumulator block are four consecutive ones (the bias and critical-query reads of the epilogues)."""
import numpy as np
import pytest

QD = 128
F2_CHUNK_F4 = 4 * 2 * 64


def unit_of(ub, m):
    return 32 * (ub >> 1) + 16 * (m >> 3) + 8 * (ub & 1) + (m & 7)


def frag_map(nk1, chunk, ub, lane, e):
    """f3_frag_map: (unit, k) of element e of lane `lane` of the fragment (chunk, ub); the same for both planes."""
    m, g = lane & 15, lane >> 4
    if_w1 = 32 * chunk + 8 * g + e
    if_w2 = 32 * (chunk - nk1) + 16 * (g >> 1) + 4 * (g & 1) + (e & 3) + 8 * (e >> 2)
    return unit_of(ub, m), np.where(chunk < nk1, if_w1, if_w2)


def frag_slot(chunk, ub, plane, lane):
    m, g = lane & 15, lane >> 4
    return (2 * chunk + (g >> 1)) * F2_CHUNK_F4 + ((ub >> 1) * 2 + plane) * 64 + 32 * (g & 1) + (unit_of(ub, m) & 31)


def f2_image_content(nks, slot, e):
    """k_pack_agg_f2: 16-byte slot [s][t][p][lane (l31, hi)], element e.  Chunk s < nks holds plane p of
    W1[32 t + l31][16 s + 8 hi + e]; chunk nks + 2 tt + sx holds plane p of W2[32 t + l31][32 tt + 16 sx + (e & 3) + 8 (e >> 2) + 4 hi]."""
    ln = slot % 64
    p = (slot // 64) % 2
    t = (slot // 128) % 4
    s = slot // F2_CHUNK_F4
    l31, hi = ln & 31, ln >> 5
    st = s - nks
    k = np.where(s < nks, 16 * s + 8 * hi + e, 32 * (st >> 1) + 16 * (st & 1) + (e & 3) + 8 * (e >> 2) + 4 * hi)
    return 32 * t + l31, k, p


def _grid(c0, c1):
    return np.meshgrid(np.arange(c0, c1), np.arange(8), np.arange(2), np.arange(64), np.arange(8), indexing="ij")


@pytest.mark.parametrize("K", [128, 256, 384, 512])
def test_every_w1_element_once(K):
    nk1 = K // 32
    chunk, ub, plane, lane, e = _grid(0, nk1)
    unit, k = frag_map(nk1, chunk, ub, lane, e)
    assert unit.min() == 0 and unit.max() == QD - 1 and k.min() == 0 and k.max() == K - 1
    count = np.zeros((QD, K, 2), dtype=np.int64)
    np.add.at(count, (unit.ravel(), k.ravel(), plane.ravel()), 1)
    assert np.array_equal(count, np.ones_like(count))


@pytest.mark.parametrize("K", [128, 256, 384, 512])
def test_every_w2_element_once(K):
    nk1 = K // 32
    chunk, ub, plane, lane, e = _grid(nk1, nk1 + 4)
    unit, k = frag_map(nk1, chunk, ub, lane, e)
    assert unit.min() == 0 and unit.max() == QD - 1 and k.min() == 0 and k.max() == QD - 1
    count = np.zeros((QD, QD, 2), dtype=np.int64)
    np.add.at(count, (unit.ravel(), k.ravel(), plane.ravel()), 1)
    assert np.array_equal(count, np.ones_like(count))


@pytest.mark.parametrize("K", [128, 256, 384, 512])
def test_fragments_are_slots_of_the_packed_image(K):
    nk1 = K // 32
    chunk, ub, plane, lane, e = _grid(0, nk1 + 4)
    slot = frag_slot(chunk, ub, plane, lane)
    one = slot[..., 0]
    assert np.array_equal(np.sort(one.ravel()), np.arange((2 * nk1 + 8) * F2_CHUNK_F4))   # every slot in front of the trailer, once
    unit, k = frag_map(nk1, chunk, ub, lane, e)
    u2, k2, p2 = f2_image_content(2 * nk1, slot, e)
    assert np.array_equal(u2, unit) and np.array_equal(k2, k) and np.array_equal(p2, plane)


def test_w2_k_order_is_the_hidden_cut_order():
    """The hidden cut: accumulator block uh of wave w holds, in lane group g, the units of block rows 4g .. 4g+3; the lane
    writes the eight hidden units of a row (block uh = 0 first) as the 16 bytes at byte 64 w + 16 g of the row's plane.  GEMM-2
    step st reads the 64 bytes at 64 st, lane group g the 16 bytes at + 16 g as its k-slots 8g .. 8g+7."""
    pos_unit = np.full(QD, -1)                     # fp16 position in the row -> hidden unit
    for w in range(4):
        for g in range(4):
            units = [unit_of(2 * w + uh, 4 * g + e) for uh in range(2) for e in range(4)]
            assert units[1:4] == [units[0] + 1, units[0] + 2, units[0] + 3] and units[4:] == [u + 8 for u in units[:4]]
            for i, u in enumerate(units):
                pos_unit[(64 * w + 16 * g) // 2 + i] = u
    assert sorted(pos_unit.tolist()) == list(range(QD))
    nk1 = 16
    for st in range(4):
        for lane in range(64):
            g = lane >> 4
            for e in range(8):
                _, k = frag_map(nk1, nk1 + st, 0, lane, e)
                assert int(k) == pos_unit[(64 * st + 16 * g) // 2 + e]
