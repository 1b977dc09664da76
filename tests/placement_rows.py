"""The rows of map_locate that walk the placement gate test by test (relocate_defs.h: placement_gate), with the code each must draw
WRITTEN BY HAND from the definition.  pose_relocate (tests/test_relocate_cpu.py) and link_place (tests/test_merge_cpu.py) both feed them to
their reference and to their host program: one gate, so one row draws one code from either op wherever the holder's own guard passes."""
import mosaic_ref as mref
import relocate_ref as lref

MAX_MEAN, RATIO = 16, 800
HOLDER = mref.affine_pose(1.01, 0.02, -0.02, 0.99, 12, -5)        # (to, back): the state's two poses, or the link's two affines
WILD = ([HOLDER[0][0], 16 * mref.ONE] + HOLDER[0][2:], HOLDER[1])   # a linear entry at the pose bound: the holder itself is unusable
EDGE = mref.affine_pose(1, 0, 0, 1, 16380, 0)                      # in bounds, and four more pixels leave them


def gate_rows():
    """(name, found, holder, code): each row passes every test in front of the one it names."""
    fr = lref.found_row
    second = (5, 5, 400, 20)                                        # mean 20 against the best's 2: far from a tie
    rows = [("no placement", fr(lref.FOUND_NONE, n=0), HOLDER, 2), ("a bad geometry", fr(lref.FOUND_BAD_GEOM, n=0), HOLDER, 6),
            ("a status that is none", fr(9, sad=40, n=20), HOLDER, 6), ("the holder out of bounds", fr(sad=40, n=20), WILD, 6),
            ("n of 0", fr(sad=0, n=0), HOLDER, 6), ("n past 65536", fr(sad=0, n=65537), HOLDER, 6), ("a negative sum", fr(sad=-1, n=20), HOLDER, 6),
            ("a sum over 255 n", fr(sad=255 * 20 + 1, n=20), HOLDER, 6), ("u past the sides", fr(u=16385, sad=40, n=20), HOLDER, 6),
            ("v past the sides", fr(v=-16385, sad=40, n=20), HOLDER, 6), ("a runner-up of no cells", fr(sad=40, n=20, second=(5, 5, 0, 0)), HOLDER, 6),
            ("a runner-up's sum over 255 n", fr(sad=40, n=20, second=(5, 5, 255 * 20 + 1, 20)), HOLDER, 6),
            ("the mean over the limit", fr(sad=MAX_MEAN * 20 + 1, n=20, second=second), HOLDER, 3),
            ("the mean at the limit", fr(sad=MAX_MEAN * 20, n=20, second=(5, 5, 255 * 20, 20)), HOLDER, 0),
            ("the ratio over the limit", fr(sad=41, n=20, second=(9, 0, 50, 20)), HOLDER, 4),       # 1000 x 41 x 20 > 800 x 50 x 20
            ("the ratio at the limit", fr(sad=40, n=20, second=(9, 0, 50, 20)), HOLDER, 0),         # 1000 x 40 x 20 = 800 x 50 x 20
            ("u at the sides: the move leaves the bounds", fr(u=16384, sad=40, n=20), HOLDER, 7), ("four pixels too far", fr(u=2, sad=0, n=5), EDGE, 7),
            ("placed", fr(u=-3, v=2, sad=40, n=20, second=second), HOLDER, 0), ("placed without a runner-up", fr(u=1, sad=0, n=7), HOLDER, 0)]
    assert sorted({r[3] for r in rows}) == [0, 2, 3, 4, 6, 7]
    return rows
