"""The trims of the fast list kernels on the host side (kernels.h: trims_mul24, trims_fold_rgb): the LDS a launch asks
for with the fold's colour table in it, and the bounds the 24-bit address products take for granted.  No GPU involved.

The constants are those of the sources, restated: the test holds the library to the numbers, not to its own headers."""
import common
import fast_trim_worlds as ft
import rtmi

LDS_PER_CU = 160 * 1024   # a compute unit's LDS on gfx950
WAVES_PER_SIMD = 6        # what the list kernels are built for: six workgroups of 256 lanes per compute unit
MAT_REC = 32              # sizeof(MatRec)
FOLD_RGB_OFF, FOLD_RGB_BYTES = 512, 256  # kFoldRgbOff, kFoldRgbBytes (kernels.h)
TRI_PTS = 48              # sizeof(TriPts)
LDS_PAIRS = 128           # kLdsPairs (scene_dev.h)
MAX_DEPTH = 64            # RTMI_MAX_DEPTH (include/rtmi.h)
MAX_THREADS = 1024        # lanes of the largest workgroup any device takes (the list kernels are launched with 256 at most)


def _cornell():
    return common.build_scene(rtmi.SceneBuilder(common.scene_seed("cornell_box")), "cornell_box", 1.0)


def _builder(fill, seed=13):
    b = rtmi.SceneBuilder(seed)
    fill(b)
    return b


def test_c2_fits_six_workgroups_with_the_colour_table():
    """C2: cornell_box at depth 50 in workgroups of 256 lanes.  Its four materials take 128 bytes; the table sits at its
    fixed place behind the largest table nibble ids can name, and the id stack behind it."""
    lds = _cornell().render_lds_bytes(50, 256)
    print("cornell_box, depth 50, 256 lanes: %d bytes of LDS per workgroup" % lds)
    assert 0 < lds and WAVES_PER_SIMD * lds <= LDS_PER_CU, lds
    assert FOLD_RGB_OFF == 16 * MAT_REC and FOLD_RGB_BYTES == 16 * 16
    # the layout in front of the staged records: table, then 25 rows of 256 nibble pairs
    assert lds >= FOLD_RGB_OFF + FOLD_RGB_BYTES + 25 * 256, lds


def test_the_table_is_the_nibble_launches_alone():
    """Sixteen materials have the table in front of their id stack; a seventeenth turns the stack into bytes and the
    table away: twice the stack, no table, and the material table one record longer."""
    cornell_pairs, pair_bytes = 18, 2 * TRI_PTS + 2 * 16  # two TriPts and two TriNrm records per pair
    shared = _cornell().render_lds_bytes(50, 256) - (FOLD_RGB_OFF + FOLD_RGB_BYTES + 25 * 256 + cornell_pairs * pair_bytes)
    assert shared > 0 and shared % 1024 == 0, shared  # the four waves' regions of the shared candidate tests
    with16, with17 = (_builder(ft.box(n)).render_lds_bytes(50, 256) for n in (16, 17))
    assert with16 == FOLD_RGB_OFF + FOLD_RGB_BYTES + 25 * 256 + 16 * pair_bytes + shared, with16
    assert with17 == 17 * MAT_REC + 50 * 256 + 17 * pair_bytes + shared, with17


def test_address_products_fit_24_bits():
    """v_mul_u32_u24 multiplies the low 24 bits of its operands: both operands and the product must fit them for the
    largest list whose records are staged (one pair of padding behind it), the deepest id stack and the largest
    workgroup."""
    limit = 1 << 24
    records = 2 * LDS_PAIRS + 2
    assert records < limit and TRI_PTS < limit and records * TRI_PTS < limit
    assert MAX_DEPTH < limit and MAX_THREADS < limit and MAX_DEPTH * MAX_THREADS < limit
    # the longest staged list is what the library stages: one pair more and the records stay in global memory
    assert _builder(ft.full_list()).pair_slabs()[0].shape[0] == LDS_PAIRS + 1
