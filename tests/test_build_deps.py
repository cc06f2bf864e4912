"""build_hip's incremental rule: a unit recompiles exactly when a file its hipcc depfile lists is newer than its object.
Pure file-system checks (no hipcc, no GPU)."""
import os

import __graft_entry__ as ge


def _touch(path, mtime):
    with open(path, "a"):
        pass
    os.utime(path, (mtime, mtime))


def _unit(tmp_path):
    """An object, its depfile (continued over several lines, absolute paths, one with an escaped space) and the files it lists."""
    src, hdr, other = tmp_path / "k.hip", tmp_path / "inc dir" / "a.h", tmp_path / "b.h"
    hdr.parent.mkdir()
    obj, dep = tmp_path / "k.hip.o", tmp_path / "k.hip.o.d"
    for p in (src, hdr, other):
        _touch(p, 1000)
    _touch(obj, 2000)
    dep.write_text("%s: %s \\\n  %s \\\n  %s\n" % (obj, src, str(hdr).replace(" ", "\\ "), other))
    return obj, dep, src, hdr, other


def test_depfile_lists_every_prerequisite(tmp_path):
    obj, dep, src, hdr, other = _unit(tmp_path)
    assert ge.depfile_paths(str(dep)) == [str(src), str(hdr), str(other)]


def test_fresh_unit_is_not_stale(tmp_path):
    obj, dep, *_ = _unit(tmp_path)
    assert not ge.unit_is_stale(str(obj), str(dep))


def test_listed_header_newer_than_object_makes_the_unit_stale(tmp_path):
    obj, dep, src, hdr, other = _unit(tmp_path)
    _touch(hdr, 3000)
    assert ge.unit_is_stale(str(obj), str(dep))


def test_unlisted_header_leaves_the_unit_alone(tmp_path):
    obj, dep, *_ = _unit(tmp_path)
    _touch(tmp_path / "c.h", 3000)
    assert not ge.unit_is_stale(str(obj), str(dep))


def test_missing_object_depfile_or_listed_file_makes_the_unit_stale(tmp_path):
    obj, dep, src, hdr, other = _unit(tmp_path)
    os.remove(other)
    assert ge.unit_is_stale(str(obj), str(dep))
    assert ge.unit_is_stale(str(obj), str(tmp_path / "none.d"))
    assert ge.unit_is_stale(str(tmp_path / "none.o"), str(dep))
