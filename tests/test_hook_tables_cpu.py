"""The binding's walk over the library's nine hook tables (_lib._Library), table by table: every member resolves to its slot of the nested
fs_hook_tables8 struct, and a table whose magic is not the expected one stops the lookups of its own members and of every later
table's, with the message that names it, while the tables in front of it stay usable.  Needs the built library, no GPU."""
import ctypes

import pytest

from flood_uav_video_segmentation_amd import _lib

NAMES = [_lib.hook_names, _lib.ext_hook_names, _lib.ext2_hook_names, _lib.ext3_hook_names, _lib.ext4_hook_names, _lib.ext5_hook_names,
         _lib.ext6_hook_names, _lib.ext7_hook_names, _lib.ext8_hook_names]
MEMBER = ["test", "ext", "ext2", "ext3", "ext4", "ext5", "ext6", "ext7", "ext8"]
COUNT = [None, None, "two", "three", "four", "five", "six", "seven", "eight"]    # "the library's first ... hook tables"
NTH = [None, None, "second", "third", "fourth", "fifth", "sixth", "seventh", "eighth"]


def fresh_library():
    lib = _lib._Library(ctypes.CDLL(_lib.LIB_PATH))
    lib._cdll.fs_test_hooks.restype = ctypes.c_void_p
    return lib


def address(fn):
    return ctypes.cast(fn, ctypes.c_void_p).value


def table_of(all8, n):
    """Table n read through the nesting itself: fs_hook_tables8.base7.base6 ... down to the struct that ends with it."""
    s = all8
    for level in range(8, max(n, 1), -1):
        s = getattr(s, "base" + (str(level - 1) if level > 2 else ""))
    return getattr(s, MEMBER[n])


def test_the_nine_tables_are_the_ones_the_tests_pin():
    assert [len(names()) for names in NAMES] == [38, 2, 14, 1, 1, 1, 1, 2, 4]
    assert len({name for names in NAMES for name in names()}) == 64                                      # no name lives in two tables


@pytest.mark.parametrize("n", range(9))
def test_every_member_resolves_to_its_slot(n):
    lib = fresh_library()
    all8 = ctypes.cast(lib._cdll.fs_test_hooks(), ctypes.POINTER(_lib.FsHookTables8)).contents
    table = table_of(all8, n)
    for name in NAMES[n]():
        fn = getattr(lib, "fs_" + name)
        assert address(fn) == address(getattr(table, name)) and address(fn)
        assert getattr(lib, "fs_" + name) is fn and "fs_" + name in vars(lib)                            # resolved once, then an attribute
    assert address(lib.fs_test_hooks) == address(lib._cdll.fs_test_hooks) and lib.fs_version() == _lib.load().fs_version()   # exported symbols
    with pytest.raises(AttributeError):
        lib.fs_no_such_member


@pytest.mark.parametrize("n", range(2, 9))
def test_a_table_with_another_magic_stops_itself_and_every_later_table(monkeypatch, n):
    magic = f"EXT{n}_MAGIC"
    lib = fresh_library()
    monkeypatch.setattr(_lib, magic, getattr(_lib, magic) + 1)                                           # read when the lookup happens
    for name in NAMES[n]():
        with pytest.raises(RuntimeError, match=f"the library has no {NTH[n]} extension table \\(fs_{name} is missing\\)"):
            getattr(lib, "fs_" + name)
    for later in range(n + 1, 9):
        word = f"the library's first {COUNT[later]} hook tables are not the ones this binding knows \\(fs_{NAMES[later]()[0]} is missing\\)"
        with pytest.raises(RuntimeError, match=word):
            getattr(lib, "fs_" + NAMES[later]()[0])
    for earlier in range(n):
        assert all(address(getattr(lib, "fs_" + name)) for name in NAMES[earlier]())
    monkeypatch.undo()
    assert all(address(getattr(lib, "fs_" + name)) for m in range(n, 9) for name in NAMES[m]())        # nothing was cached from the refusals
    # a table's checks run once per library: once one member has resolved, the table's other members do not look at the magic again
    other = fresh_library()
    assert address(getattr(other, "fs_" + NAMES[n]()[0]))
    monkeypatch.setattr(_lib, magic, getattr(_lib, magic) + 1)
    assert all(address(getattr(other, "fs_" + name)) for name in NAMES[n]())
