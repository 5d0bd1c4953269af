"""The assembly generator and its lint (csrc/asm) as the CPU tests of the generated streams use them."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASM = os.path.join(ROOT, "mingraph-unet_amd", "csrc", "asm")


def load(name):
    """a fresh copy of csrc/asm/<name>.py: a fault seeded in it reaches no other test"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(ASM, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def generate(*flags, patch=None):
    """(the stream `gen_wino_cp.py FLAGS OUT.s` writes, the generator module); patch(module) may seed a fault first"""
    assert set(flags) <= {"--head"}
    gen = load("gen_wino_cp")
    if patch:
        patch(gen)
    return gen.generate("--head" in flags), gen


def run_cli(tmp_path, *flags):
    """the stream the command line `gen_wino_cp.py FLAGS OUT.s` writes (what the Makefile runs)"""
    out = tmp_path / ("k" + "".join(flags) + ".s")
    subprocess.run([sys.executable, os.path.join(ASM, "gen_wino_cp.py"), *flags, str(out)], check=True)
    return out.read_text()
