"""The header list of aod_meh_hua_amd/build.py against the sources, without a build or a device: build.headers() is the one list behind
source_digest() (the tag of a PMC profile's build) and needs_build() (the rebuild check), so every header a source includes must be in
it -- a header outside it gives a stale library after an edit and a digest that no longer names the build."""
import os
import re
import shutil

from aod_meh_hua_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _norm(paths):
    return {os.path.realpath(p) for p in paths}


def test_every_quoted_include_is_a_listed_header():
    listed = _norm(build.headers())
    files = [os.path.join(build.CSRC, f) for f in sorted(os.listdir(build.CSRC)) if f.endswith(('.hip', '.cpp', '.h'))]
    assert os.path.join(build.CSRC, 'tile_prims.h') in files and len(files) > 30
    seen = 0
    for f in files:
        for name in INCLUDE.findall(open(f).read()):
            assert not os.path.isabs(name), (f, name)
            target = os.path.realpath(os.path.join(os.path.dirname(f), name))
            assert os.path.isfile(target), f'{f}: #include "{name}" does not resolve'
            assert target in listed, f'{f}: #include "{name}" is not in build.headers()'
            seen += 1
    assert seen >= len(files)      # (every file includes at least one project header: the pattern did find them)
    assert os.path.realpath(os.path.join(build.HERE, '..', 'include', 'aod_hip.h')) in listed


def test_headers_are_the_h_files_of_csrc_sorted():
    hs = build.headers()
    in_csrc = [h for h in hs if os.path.dirname(h) == build.CSRC]
    assert in_csrc == sorted(os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC) if f.endswith('.h'))
    assert len(hs) == len(in_csrc) + 1 and os.path.basename(hs[-1]) == 'aod_hip.h'


def test_digest_follows_one_byte_of_tile_prims(tmp_path, monkeypatch):
    csrc = tmp_path / 'csrc'
    shutil.copytree(build.CSRC, csrc)
    monkeypatch.setattr(build, 'CSRC', str(csrc))
    assert str(csrc / 'tile_prims.h') in build.headers()
    before = build.source_digest()
    assert before == build.source_digest()
    p = csrc / 'tile_prims.h'
    data = bytearray(p.read_bytes())
    data[len(data) // 2] ^= 1
    p.write_bytes(bytes(data))
    assert build.source_digest() != before
