"""csrc/drt_fold.h: the draw with the first step of its hash round folded out of the lanes' work -- fold16 of the index hash on the scalar
unit, fold16 of the key once per sample -- gives the bits of include/drt_hip.h's drt_rng_combine, the definition.  A stand-alone program
(tests/cpp/fold_kat.cpp) compares them over every index hash of the form a << 16 | a, four corner words and 10^6 pseudo-random ones, each
against 69 keys; once as an ordinary build, once as a plain executable under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_folded_draw_known_answers(tmp_path, flags):
    exe = str(tmp_path / "fold_kat")
    subprocess.run(["g++", *flags, "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "fold_kat.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.stdout, p.stderr)
