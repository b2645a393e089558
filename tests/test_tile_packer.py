"""The length-balanced tile packer (id-grec_amd/csrc/idg_tile_packer.h) as a stand-alone host program under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/tile_packer_check.cpp states what it asserts), on built-in degree
lists and on the yelp2018-shape list of idgrec_amd.synth.generate.

Lane-group utilisation = sum of the vrows' rounds / sum over tiles of 16 x the tile's list-schedule makespan, rounds =
max(1, ceil(len / 8)).  The consecutive packing scores 0.379 on the yelp2018 list (5,321 tiles), a crude greedy 0.616;
the packer has to reach 0.55 in no more tiles than the consecutive packing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_UTILISATION = 0.55


def test_packer_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    import idgrec_amd.synth as S

    U, I, E = S.SHAPES["yelp2018"]
    users, items = S.generate(U, I, E, seed=0)
    deg = np.concatenate([np.bincount(users, minlength=U), np.bincount(items, minlength=I)])
    band = np.concatenate([np.zeros(U, dtype=np.int64), np.ones(I, dtype=np.int64)])  # user rows / item rows
    lst = tmp_path / "yelp2018.txt"
    with open(lst, "w") as f:
        f.write("%d\n" % len(deg))
        f.write("\n".join("%d %d" % (l, b) for l, b in zip(deg.tolist(), band.tolist())))
        f.write("\n")
    exe = str(tmp_path / "tile_packer_check")
    build = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "id-grec_amd", "csrc"),
                            os.path.join(ROOT, "tests", "tile_packer_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("this g++ has no sanitizer runtimes")
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe, str(lst), repr(MIN_UTILISATION)], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    print(run.stdout)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().endswith("ok")
