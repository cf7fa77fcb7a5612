"""CPU: the packed block of the fused batch pipelines (csrc/packed_block.h) -- host/packed_block_check.cpp built with
-fsanitize=address,undefined and run as a stand-alone program.  It includes that header alone, so it needs no device and
no library.  The program rebuilds the section lists of mixed_batch.hip, dantzig.hip and dense_iter.hip from the same
counts and checks zones, alignment, overlap, the refused out-of-order add and a gather / upload / "kernel" / read-back /
scatter round trip through blocks of exactly host_bytes() and total_bytes()."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "eggshell_amd", "csrc")


def test_packed_block_layouts_under_sanitizers(tmp_path):
    host = os.path.join(ROOT, "eggshell_amd", "host")
    out = str(tmp_path / "packed_block_check")
    res = subprocess.run(["make", "-B", "-C", host, "packed_block_check", "PACKED_CHECK_OUT=" + out], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "-fsanitize=address,undefined" in res.stdout and "warning" not in res.stderr, (res.stdout[-2000:], res.stderr[-2000:])
    run = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "packed_block_check: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-2000:])


def test_packed_block_header_is_host_only():
    text = open(os.path.join(CSRC, "packed_block.h")).read()
    assert "hip" not in re.sub(r"//.*", "", text).lower()
    check = open(os.path.join(ROOT, "eggshell_amd", "host", "packed_block_check.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', check) == ["../csrc/packed_block.h"]


def test_the_three_pipelines_lay_their_block_out_with_it():
    """No hand-written offset chain or rounding lambda is left beside the builder, and the entries' hooks are made in one
    place."""
    for name in ("mixed_batch.hip", "dantzig.hip", "dense_iter.hip"):
        text = open(os.path.join(CSRC, name)).read()
        assert '#include "packed_block.h"' in text and "PackedBlock blk;" in text, name
    for name in os.listdir(CSRC):
        path = os.path.join(CSRC, name)
        if not os.path.isfile(path):
            continue
        text = open(path, errors="replace").read()
        assert not re.search(r"o_[a-zA-Z]+ = o_", text), name
        assert not re.search(r"\bup(8|16)\b", text), name
    assert open(os.path.join(CSRC, "dense.cpp")).read().count("LaunchHooks hooks;") == 1
