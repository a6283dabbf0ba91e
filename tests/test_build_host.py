"""The build recipe of _lib.py checked without a compiler: what build() would compile, where it links to and how many compiles it runs
at a time (its hipcc processes are replaced by a recorder), what it takes as sources and staleness inputs, and the reader of the
compiler's ``amdhsa.kernels`` notes on a canned block."""
import os
import re
import shutil
import subprocess
import threading

import pytest

import msod_amd  # noqa: F401
from msod_amd import _lib


@pytest.fixture
def csrc_copy(tmp_path, monkeypatch):
    """A package directory of its own for _lib: a fresh copy of csrc/ (new mtimes: every object is stale against it), the object cache
    and the library all under tmp_path; nothing in the real package moves, and the library this process has loaded stays loaded."""
    dst = tmp_path / "pkg" / "csrc"
    shutil.copytree(_lib.CSRC, dst, copy_function=shutil.copy)
    monkeypatch.setattr(_lib, "CSRC", str(dst))
    monkeypatch.setattr(_lib, "_HERE", str(tmp_path / "pkg"))
    monkeypatch.setattr(_lib, "BUILT_LIB", str(tmp_path / "pkg" / "libcft_hip.so"))
    monkeypatch.setattr(_lib, "_lib", _lib._lib)
    return dst


def _record(monkeypatch, cap):
    """Replace subprocess.Popen: commands are recorded, none runs.  The first ``cap`` processes end only once ``cap`` of them are alive
    together (so the limit is reached, not merely respected); the peak of live processes is kept."""
    class Recorder:
        cmds, alive, peak = [], 0, 0
        lock, gate = threading.Lock(), threading.Barrier(cap)

        def __init__(self, cmd, **kw):
            with Recorder.lock:
                self.n = len(Recorder.cmds)
                Recorder.cmds.append(list(cmd))
                Recorder.alive += 1
                Recorder.peak = max(Recorder.peak, Recorder.alive)

        def wait(self):
            if self.n < cap:
                Recorder.gate.wait(timeout=20)
            with Recorder.lock:
                Recorder.alive -= 1
            return 0

    monkeypatch.setattr(subprocess, "Popen", Recorder)
    return Recorder


def test_build_links_in_tree_whatever_cft_hip_lib_says(csrc_copy, tmp_path, monkeypatch):
    other = tmp_path / "other" / "libcft_hip.so"
    monkeypatch.setenv("CFT_HIP_LIB", str(other))
    monkeypatch.setattr(_lib, "LIB_PATH", str(other))                # what the variable does at import
    rec = _record(monkeypatch, 1)
    in_tree = _lib.BUILT_LIB
    assert _lib.build() == in_tree
    *compiles, link = rec.cmds
    assert link[link.index("-o") + 1] == in_tree and "-shared" in link
    assert not any(str(other) in word for cmd in rec.cmds for word in cmd) and not other.exists()
    # one compile per source with the one flag list, every object linked
    assert [c[c.index("-c") + 1] for c in compiles] == _lib.sources() and len(compiles) >= 23
    assert all(c[1:1 + len(_lib.HIPCC_FLAGS)] == _lib.HIPCC_FLAGS for c in compiles)
    assert [c[c.index("-o") + 1] for c in compiles] == link[link.index("-o") + 2:]


def test_other_output_or_flags_leave_the_object_cache_alone(csrc_copy, tmp_path, monkeypatch):
    rec = _record(monkeypatch, 1)
    cache = os.path.join(_lib._HERE, "build") + os.sep
    monkeypatch.setattr(_lib, "_lib", "the loaded library")
    assert _lib.build(out=str(tmp_path / "x.so"), extra_flags=("-DPROBE=1",)) == str(tmp_path / "x.so")
    *compiles, link = rec.cmds
    assert len(compiles) == len(_lib.sources()) and all("-DPROBE=1" in c for c in compiles)
    assert not any(word.startswith(cache) for cmd in rec.cmds for word in cmd)
    assert link[link.index("-o") + 1] == str(tmp_path / "x.so") and "-DPROBE=1" in link
    assert _lib._lib == "the loaded library" and not os.path.exists(cache)      # load() keeps what it loaded: that build is not its library


@pytest.mark.parametrize("max_jobs, cap", [("64", 16), ("4", 4), ("0", 1)])
def test_never_more_compiles_at_once_than_allowed(csrc_copy, monkeypatch, max_jobs, cap):
    monkeypatch.setenv("MAX_JOBS", max_jobs)
    rec = _record(monkeypatch, cap)
    _lib.build()
    assert len(rec.cmds) > cap and rec.peak == cap and rec.alive == 0


def test_a_file_dropped_into_csrc_is_built_and_watched(csrc_copy, monkeypatch):
    for name in ("zz_new.hip", "zz_new.h", "zz_new.inc"):
        (csrc_copy / name).write_text("\n")
    assert str(csrc_copy / "zz_new.hip") in _lib.sources()
    assert {str(csrc_copy / "zz_new.h"), str(csrc_copy / "zz_new.inc"), _lib.HEADER} <= set(_lib.staleness_inputs())
    rec = _record(monkeypatch, 1)
    _lib.build()
    assert any(str(csrc_copy / "zz_new.hip") in cmd for cmd in rec.cmds[:-1])
    assert any(word.endswith("zz_new.o") for word in rec.cmds[-1])


def test_every_quoted_include_is_a_staleness_input():
    watched = {os.path.realpath(p) for p in _lib.staleness_inputs()}
    files = _lib.sources() + _lib.staleness_inputs()
    seen = 0
    for path in files:
        with open(path) as fh:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), flags=re.M):
                seen += 1
                assert os.path.realpath(os.path.join(os.path.dirname(path), name)) in watched, (path, name)
    assert seen >= len(_lib.sources())


_ENTRY_A = """  - .agpr_count:     128
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: 0
    .name:           _Z6kern_aPf
    .private_segment_fixed_size: 16
    .sgpr_spill_count: 3
    .symbol:         _Z6kern_aPf.kd
    .vgpr_count:     96
    .vgpr_spill_count: 0
"""
_ENTRY_C = """  - .args:
      - .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .language:       OpenCL C
    .name:           _Z6kern_cPf
    .vgpr_count:     7
"""
_ENTRY_B = """  - .name:           _Z6kern_bPf
    .vgpr_spill_count: 2
    .vgpr_count:     512
    .args:
      - .offset:         0
        .size:           4
        .value_kind:     by_value
    .sgpr_spill_count: 0
    .private_segment_fixed_size: 0
    .group_segment_fixed_size: 65536
    .agpr_count:     0
    .symbol:         _Z6kern_bPf.kd
"""


def test_kernel_notes_do_not_depend_on_key_order():
    want = {"_Z6kern_aPf": {"agpr_count": 128, "group_segment_fixed_size": 0, "private_segment_fixed_size": 16, "sgpr_spill_count": 3,
                            "vgpr_count": 96, "vgpr_spill_count": 0},
            "_Z6kern_bPf": {"agpr_count": 0, "group_segment_fixed_size": 65536, "private_segment_fixed_size": 0, "sgpr_spill_count": 0,
                            "vgpr_count": 512, "vgpr_spill_count": 2},
            "_Z6kern_cPf": {"vgpr_count": 7}}                    # an entry whose first key has no value on its line
    for entries in (_ENTRY_A + _ENTRY_B + _ENTRY_C, _ENTRY_C + _ENTRY_B + _ENTRY_A):
        asm = "\ts_endpgm\n\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + entries + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n"
        assert _lib.kernel_notes(asm) == want


def test_device_asm_compiles_a_source_once_whatever_holds_the_flags(monkeypatch):
    runs = []
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: runs.append(cmd) or subprocess.CompletedProcess(cmd, 0, "listing", ""))
    src = os.path.join(_lib.CSRC, "no_such_source.hip")
    assert _lib.device_asm(src, ["-DX=1"]) == _lib.device_asm(src, ("-DX=1",)) == "listing"
    assert len(runs) == 1 and runs[0][1:1 + len(_lib.HIPCC_FLAGS)] == _lib.HIPCC_FLAGS and "-DX=1" in runs[0]
    _lib._device_asm.cache_clear()
