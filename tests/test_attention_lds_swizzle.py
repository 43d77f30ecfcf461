"""Host enumeration of the LDS bank slots that attention_f16x2.hip's ds_read_b128 fragment reads touch (no GPU needed).

ds_read_b128 is served in four non-contiguous 16-lane groups and the bank of byte address a is (a / 4) % 64, so a group is
conflict-free when its sixteen 16-B reads fall on sixteen different 16-B slots of the 256-B bank row. The formulas below are the
kernel's (its header comment): lane l = 16 g + i reads, for S^T = K Q^T, K row 16 (i >> 3) + (i & 7) + 8 kb at logical chunk
4 st + g, and for O^T += V^T P^T, V^T row 16 db + i at logical chunk g; a chunk c of a row lies at c ^ swizzle(row).
"""
GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS += [[l + 32 for l in grp] for grp in GROUPS]


def _k_slot(lane, kb, st, swizzle):
    g, i = lane >> 4, lane & 15
    row = 16 * (i >> 3) + (i & 7) + 8 * kb
    return (row * 256 + ((4 * st + g) ^ swizzle(row)) * 16) // 16 % 16


def _vt_slot(lane, db, swizzle):
    g, i = lane >> 4, lane & 15
    row = 16 * db + i
    return (row * 64 + (g ^ swizzle(row)) * 16) // 16 % 16


def _worst(slot):
    return max(max(map([slot(l) for l in grp].count, range(16))) for grp in GROUPS)


def test_k_swizzle_is_conflict_free_for_every_group_and_step():
    sw = lambda r: (r & 7) | ((r >> 1) & 8)
    for kb in range(2):
        for st in range(4):
            assert _worst(lambda l: _k_slot(l, kb, st, sw)) == 1, (kb, st)
    # the swizzle of the 32x32x16 form, c ^ (row & 15), is 2-way under the key permutation: why it changed
    assert _worst(lambda l: _k_slot(l, 0, 0, lambda r: r & 15)) == 2


def test_vt_swizzle_is_conflict_free_for_every_group_and_block():
    sw = lambda r: -(r >> 2) & 3
    for db in range(8):
        assert _worst(lambda l: _vt_slot(l, db, sw)) == 1, db
    assert _worst(lambda l: _vt_slot(l, 0, lambda r: (r >> 2) & 3)) == 2


def test_key_of_register_matches_the_vt_chunk_order():
    """C register r of lane group g in key block kb is A row 4 g + r, i.e. key 16 (g >> 1) + 4 (g & 1) + 8 kb + r; position j = 4 kb + r
    of V^T chunk g (columns = rows with index bits 2 and 3 swapped) must be the same key"""
    for g in range(4):
        for kb in range(2):
            for r in range(4):
                i = 4 * g + r
                key = 16 * (i >> 3) + (i & 7) + 8 * kb
                assert key == 16 * (g >> 1) + 4 * (g & 1) + 8 * kb + r
                p = 8 * g + 4 * kb + r                                   # V^T column inside the 32-key tile
                assert key == (p & ~12) | ((p & 4) << 1) | ((p & 8) >> 1)
