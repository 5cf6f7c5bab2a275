"""CPU-only sanitizer build of the verify intermediates' layout
(haskoin-node_amd/csrc/hkv_layout.h: the field table of `im` and `aux` and the
live set of every hand-off between launches). tests/im_layout.cpp includes the
header alone, so the header's own static_asserts (every pair of fields live
together shares no word row) are checked by each compile; it prints every
field's offset and length and re-runs the live-set checks at run time, under
AddressSanitizer and UndefinedBehaviorSanitizer. The default build's offsets
are pinned to literal values (the kernels, the host's buffer sizes and every
recorded profile assume them); the other knob pairs, which nothing else
compiles, must build and keep their checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (HKV_QW, HKV_GTAB_W): G windows sit on Q window boundaries, 8 <= GTAB_W <= 28
SUPPORTED = [(4, w) for w in (8, 12, 16, 20, 24, 28)] + [(5, w) for w in (10, 15, 20, 25)]
# rejected by the header's own static_asserts: none of the supported pairs is;
# these two (a G window off the Q window boundaries) show that a rejection is seen
REJECTED = [(4, 10), (5, 12)]

# the default build (QW 4, GTAB_W 20): name -> (first word row, rows)
DEFAULT = {
    "IM_FLAGS": (0, 1), "IM_QX": (1, 8), "IM_W": (9, 8), "IM_S": (17, 8), "IM_M": (27, 8), "IM_R": (35, 8),
    "IM_C": (43, 8), "IM_DIG": (51, 33), "IM_GDIG": (84, 14),
    "IM_BX": (51, 8), "IM_BY": (59, 8), "IM_BZ": (67, 8),
    "IM_NUM": (51, 8), "IM_NUMN": (59, 8), "IM_DEN": (67, 8),
    "IM_AX": (1, 8), "IM_AY": (17, 8), "IM_AZ": (25, 8), "IM_RARE_LIST": (33, 1),
    "AUX_AX": (0, 8), "AUX_AY": (8, 8), "AUX_AZ": (16, 8), "AUX_Y0": (24, 8), "AUX_FLAGS": (32, 1), "AUX_SQ": (33, 1),
}


def build(tmp_path, qw, gw):
    exe = str(tmp_path / ("im_layout_%d_%d" % (qw, gw)))
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DHKV_QW=%d" % qw,
                        "-DHKV_GTAB_W=%d" % gw, "-o", exe, os.path.join(ROOT, "tests", "im_layout.cpp")],
                       capture_output=True, text=True)
    return exe, r


def run(exe):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    head = dict(zip(lines[0].split()[0::2], map(int, lines[0].split()[1::2])))
    fields = {}
    for ln in lines[1:]:
        t = ln.split()
        if len(t) == 3:
            fields[t[0]] = (int(t[1]), int(t[2]))
    assert r.stdout.rstrip().endswith("ok 8"), r.stdout  # all eight live sets
    return head, fields


def test_default_layout_is_pinned(tmp_path):
    exe, r = build(tmp_path, 4, 20)
    assert r.returncode == 0, r.stderr
    head, fields = run(exe)
    assert head == {"QW": 4, "GTAB_W": 20, "NWIN": 33, "GWIN": 7, "IM_WORDS": 98, "AUX_WORDS": 34}
    assert fields == DEFAULT


@pytest.mark.parametrize("qw,gw", SUPPORTED)
def test_every_supported_radix_keeps_the_live_sets_disjoint(tmp_path, qw, gw):
    exe, r = build(tmp_path, qw, gw)
    assert r.returncode == 0, r.stderr  # the header's static_asserts hold
    head, fields = run(exe)
    nwin, gwin = (130 + qw - 1) // qw, (128 + gw) // gw
    assert head == {"QW": qw, "GTAB_W": gw, "NWIN": nwin, "GWIN": gwin, "IM_WORDS": 84 + 2 * gwin, "AUX_WORDS": 34}
    # only the digit fields' lengths follow the knobs; no field moves
    want = dict(DEFAULT, IM_DIG=(51, nwin), IM_GDIG=(84, 2 * gwin))
    assert fields == want
    assert all(off + ln <= head["IM_WORDS"] for name, (off, ln) in fields.items() if name.startswith("IM_"))


@pytest.mark.parametrize("qw,gw", REJECTED)
def test_a_radix_the_header_rejects_does_not_compile(tmp_path, qw, gw):
    _, r = build(tmp_path, qw, gw)
    assert r.returncode != 0
    assert "static assertion failed" in r.stderr or "static_assert" in r.stderr, r.stderr
