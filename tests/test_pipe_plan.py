"""CPU-only sanitizer build of the part plan
(haskoin-node_amd/csrc/hkv_launch_plan.h: RecPlan::part_len, n_parts, qs_slots,
part(k), part_stream / part_slot, verdict_stride_of): tests/pipe_plan.cpp, a
stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer (any
report aborts the run), checks over the four geometries of
tests/launch_plan.cpp, with the parts off and at seven part lengths, for every
n from 1 to two resident grids plus a workgroup, 2^24 and 0xFFFFFF00, that the
parts are an exact ordered cover of [0, n_pad), that a two-slot plan's part
length is aligned and both slots fit the Q scratch the plan reserves anyway,
that every field the plan had before equals the plan with parts off, that two
slots are taken exactly when they fit, and that in a model of the two-stream
schedule no part's table launch precedes the chain launch of its slot's
previous user."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_part_plan_covers_aligns_fits_and_orders_its_slots_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "pipe_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "pipe_plan.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout
    cases, piped, parts = (int(x) for x in r.stdout.split()[1:4])
    # 8 part settings x (2 * 262,144 + 256 (twice), 2 * 32,768 + 256, 2 * 65,536 + 256) batch sizes at least,
    # two-slot plans and modelled parts among them
    assert cases > 8 * 1245000 and piped > 100000 and parts > 100000
