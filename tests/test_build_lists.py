"""build.SOURCES / build.HEADERS against the files in csrc/.

needs_build() decides from these two lists whether the library is stale, and build() compiles SOURCES: a unit missing from
SOURCES is not in the library, a unit or header missing from the lists can change without a rebuild."""
import os

from camera_calibration_amd import build


def _csrc(suffix):
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith(suffix))


def test_build_lists_match_csrc():
    assert sorted(build.SOURCES) == _csrc(".hip")
    assert len(set(build.SOURCES)) == len(build.SOURCES)
    public = os.path.join("..", "..", "include", "cba.h")          # the one dependency outside csrc/
    assert public in build.HEADERS and os.path.exists(os.path.join(build.CSRC, public))
    headers = [h for h in build.HEADERS if h != public]
    assert sorted(headers) == _csrc(".h")
    assert len(set(headers)) == len(headers)
