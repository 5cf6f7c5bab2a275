"""CPU-only sanitizer build of the multisig tail's work-queue arithmetic
(haskoin-node_amd/csrc/hkv_tail_plan.h: the header hkv_ms_tail_kernel takes
its rounds, item counts, wait targets and record ranges from, and hkv_api.cpp
the sizes of the verdict words and record windows): tests/tail_plan.cpp walks
every item of a launch against a model of the allocated buffers, under
AddressSanitizer and UndefinedBehaviorSanitizer (any report aborts the run).
Checked, over the cross product of input counts, per-input densities up to
16-of-16, count residues against the window and the group, and windows of 64
records to the default: an item's wait target is the first item of its stage
and stages come in order (hash, per round emit then verify, resolve); every
candidate lies in exactly one group and every key check in exactly one chunk;
no group or chunk is empty or reaches past its round's records, its window or
the verdict words; and the number of verify items is the minimum (a round
with an empty window has no item for it)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tail_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tail_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "tail_plan.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    assert int(r.stdout.split()[1]) > 50000
