"""Compare the device code of two builds of libbgx.so kernel by kernel.

    python tools/kernel_diff.py A.so B.so

Disassembles every gfx950 code object of both libraries (tools/isa_lint.py) and compares
each function's instructions and encodings, with the addresses stripped and branch targets
written as symbol+offset, so a kernel that moved to another source file is matched with
itself.  Left out of the comparison: the literal of the s_add_u32 after an s_getpc_b64
(the pc-relative address of a constant table: it moves with the order of the functions in
the code object) and objdump's "..." padding lines.  Prints the symbols present in only
one library and, for every kernel that differs, the instruction counts; exit status 1
unless the two libraries are equal."""
from __future__ import annotations

import re
import sys

import isa_lint

ADDR = re.compile(r"\s*// [0-9A-F]+: ([0-9A-F]{8}( [0-9A-F]{8})*)")       # "// address: encoding" -> encoding
PCREL = re.compile(r"0x[0-9a-f]+|\b[0-9A-F]{8}$")        # the literal as printed (any width) and as encoded


def kernels_of(lib: str) -> dict:
    out = {}
    for obj in isa_lint.code_objects(lib):
        for name, body in isa_lint.kernels(isa_lint.disassemble(obj)):
            text = [ADDR.sub(r"  \1", ln) for ln in body if ln != "..."]
            for i in range(1, len(text)):
                if text[i - 1].startswith("s_getpc_b64") and text[i].startswith("s_add_u32"):
                    text[i] = PCREL.sub("<pcrel>", text[i])
            assert name not in out, f"{lib}: two functions named {name}"
            out[name] = text
    return out


def main():
    a, b = (kernels_of(p) for p in sys.argv[1:3])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = [(k, len(a[k]), len(b[k])) for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    names = iter(isa_lint.demangle(only_a + only_b + [k for k, _, _ in differ]))
    for _ in only_a:
        print(f"only in A: {next(names)}")
    for _ in only_b:
        print(f"only in B: {next(names)}")
    for _, na, nb in differ:
        print(f"differs ({na} -> {nb} instructions): {next(names)}")
    print(f"{len(a)} / {len(b)} functions, {len(set(a) & set(b)) - len(differ)} identical, {len(differ)} differ, "
          f"{len(only_a) + len(only_b)} unmatched")
    sys.exit(1 if only_a or only_b or differ else 0)


if __name__ == "__main__":
    main()
