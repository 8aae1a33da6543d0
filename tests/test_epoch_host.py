"""The length of the image backward's flush epochs (radfoam_amd/csrc/rf_epoch.hpp) compiled for the host: the
stand-alone program tests/host_harness/epoch_host.cpp, built with the shipped constants and with others, plainly and with
-fsanitize=undefined,address (the program has its own main: nothing is loaded into Python).  Over the whole input range --
resident rows 0..ROWS, both values of the wide bit -- epoch_steps returns only the two configured lengths, the short one
whenever a wide row is resident or more rows than the threshold are, and with the long length set to the short one it is
constant.  The program checks the same itself, and that the epoch word gives back what the waves added (exit status)."""
import os
import re
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "host_harness", "epoch_host.cpp")
_HDR = os.path.join(_HERE, "..", "radfoam_amd", "csrc", "rf_epoch.hpp")
_BUILD = os.path.join(_HERE, "host_harness", "_build")
ROWS = 256   # the largest table of the kernel (SH degree 0 and 1); degree 2 has 160 rows, degree 3 has 124


def _shipped():
    text = open(_HDR).read()
    get = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    return get("RF_CACHE_EPOCH"), get("RF_CACHE_EPOCH_LONG"), get("RF_CACHE_EPOCH_LONG_ROWS")


def _run(name, defines=(), sanitize=False):
    os.makedirs(_BUILD, exist_ok=True)
    exe = os.path.join(_BUILD, name)
    flags = ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", "-std=c++17", *flags, *["-D" + d for d in defines], "-o", exe, _SRC], check=True)
    res = subprocess.run([exe, str(ROWS)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-400:] + res.stderr[-2000:]
    assert res.stderr == ""
    lines = res.stdout.split("\n")
    config = tuple(int(x) for x in lines[0].split()[1:])
    table = {(int(r), int(w)): int(s) for _, r, w, s in (l.split() for l in lines if l.startswith("steps "))}
    return config, table


def _check(config, table, want):
    short, long_, limit = want
    assert config == (short, long_, limit, ROWS)
    assert sorted(table) == [(r, w) for r in range(ROWS + 1) for w in (0, 1)]
    for (resident, wide), steps in table.items():
        assert steps in (short, long_)
        if wide or resident > limit:
            assert steps == short
        else:
            assert steps == long_


CONFIGS = [(4, 8, 48), (4, 16, 0), (4, 16, 300), (2, 8, 159), (4, 4, 48), (8, 8, 0)]


def test_shipped_constants():
    short, long_, limit = _shipped()
    assert long_ >= short >= 1
    _check(*_run("epoch_host"), (short, long_, limit))


@pytest.mark.parametrize("short,long_,limit", CONFIGS)
def test_other_constants(short, long_, limit):
    d = ("RF_CACHE_EPOCH=%d" % short, "RF_CACHE_EPOCH_LONG=%d" % long_, "RF_CACHE_EPOCH_LONG_ROWS=%d" % limit)
    _check(*_run("epoch_host_%d_%d_%d" % (short, long_, limit), d), (short, long_, limit))


def test_long_equal_to_short_is_constant():
    short = _shipped()[0]
    _, table = _run("epoch_host_fixed", ("RF_CACHE_EPOCH_LONG=%d" % short,))
    assert set(table.values()) == {short}


def test_under_host_sanitizers():
    short, long_, limit = _shipped()
    _check(*_run("epoch_host_san", sanitize=True), (short, long_, limit))
    _, table = _run("epoch_host_san_fixed", ("RF_CACHE_EPOCH_LONG=%d" % short,), sanitize=True)
    assert set(table.values()) == {short}
