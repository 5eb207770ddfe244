"""The acceleration record of the host step path (sphx::AccelUniform, yasph2d_amd/csrc/sphx_handoff.hpp) against a model of accel[], the
velocity array and the device's verdict word: tests/accel_record_driver.cpp drives record and model through every sequence of up to
six host-side events — rigid passes (marked or not, as the velocities are), full passes, the step's begin with the take-over producer,
with another fused producer and with a prediction of its own (each adopting the pass that ran ahead or running it again), warm starts,
uploads, edits, state loads, failed calls, broken steps and debug downloads — and checks at every reader that K.a is taken from the
arguments only where the array stands for K.a over uniform, untouched velocities, and that nobody reads an array nobody wrote.  A
sanitized stand-alone program; needs no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
EVENTS = 13


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the record driver"
    exe = str(tmp_path_factory.mktemp("accel_record") / "accel_record_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "accel_record_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


def test_every_reader_finds_what_it_may_read(driver):
    rc, out, err = driver(6)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    sequences, reads, from_args, fills = (int(x) for x in out.split()[1:5])
    assert sequences == sum(EVENTS ** k for k in range(1, 7))
    # four of the thirteen events read accel[]: every position of every sequence holds each of them in one sequence of thirteen
    assert reads == 4 * sum(k * EVENTS ** (k - 1) for k in range(1, 7))
    assert 0 < from_args < reads, "K.a from the arguments is reachable"
    assert fills > 0, "the materialising fill is reachable"


def test_driver_plumbing(driver):
    """depth 2: of the 13 + 169 sequences one takes K.a from the arguments ([rigid pass] [begin take-over]) and three fill: [rigid pass]
    followed by another fused producer, by a prediction of its own or by a download."""
    rc, out, _ = driver(2)
    assert rc == 0 and out.split() == ["ok", str(EVENTS + EVENTS * EVENTS), str(4 * (1 + 2 * EVENTS)), "1", "3"]
    assert driver(0)[0] == 2 and driver(8)[0] == 2
