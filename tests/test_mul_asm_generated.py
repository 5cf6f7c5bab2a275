"""csrc/hkv_mul_asm.h is generated: the committed header is byte for byte what
tools/gen_mul_asm.py renders, so an edit to either without the other fails here."""
import importlib.util
import pathlib

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_committed_header_is_the_generators_output():
    spec = importlib.util.spec_from_file_location("gen_mul_asm", ROOT / "tools" / "gen_mul_asm.py")
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    committed = (ROOT / "haskoin-node_amd" / "csrc" / "hkv_mul_asm.h").read_bytes()
    assert gen.render().encode("utf-8") == committed
