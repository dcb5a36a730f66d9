#!/usr/bin/env python3
"""Instruction-level comparison of the kernels of two builds of libldpc_hip.so: every gfx950 code object of the
.hip_fatbin section is disassembled (llvm-objdump) and each kernel symbol of the OLD library is compared, branch
targets normalised and the zero fill between functions ("...") left out, with the same symbol in the NEW one.
Usage: tools/kernel_isa_diff.py [--rename REGEX=REPLACEMENT]... <old libldpc_hip.so> <new libldpc_hip.so>
--rename: re.sub(REGEX, REPLACEMENT) on every (mangled) symbol of the OLD library before the names are matched, for a
change that gives kernels other argument types or template arguments; several are applied in the order given.
Prints how many symbols are missing / differ / were added; exit status 1 if any old symbol is missing or differs."""
import argparse, os, re, struct, subprocess, sys, tempfile

OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"


def kernels(so):
    funcs = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat])
        b = open(fat, "rb").read()
        magic, pos, k = b"__CLANG_OFFLOAD_BUNDLE__", 0, 0
        while True:
            i = b.find(magic, pos)
            if i < 0:
                break
            n = struct.unpack_from("<Q", b, i + 24)[0]
            p = i + 32
            for _ in range(n):
                off, size, idl = struct.unpack_from("<QQQ", b, p)
                p += 24
                tid = b[p:p + idl].decode()
                p += idl
                if "gfx950" not in tid or not size:
                    continue
                co = os.path.join(tmp, "co%d.o" % k)
                k += 1
                open(co, "wb").write(b[i + off:i + off + size])
                txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", co],
                                     capture_output=True, text=True).stdout
                cur = None
                for line in txt.split("\n"):
                    m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line.strip())
                    if m:
                        cur = m.group(1)
                        funcs[cur] = []
                    elif cur and line.strip() and line.strip() != "..." and not line.startswith("Disassembly"):
                        ins = re.sub(r"//.*$", "", line).strip()
                        funcs[cur].append(re.sub(r"0x[0-9a-f]+ <[^>]*>|<[^>]*>", "<label>", ins))
            pos = i + 1
    return funcs


ap = argparse.ArgumentParser()
ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPLACEMENT")
ap.add_argument("old")
ap.add_argument("new")
args = ap.parse_args()
old, new = kernels(args.old), kernels(args.new)
for rule in args.rename:
    pat, _, repl = rule.partition("=")
    renamed = {}
    for s, body in old.items():
        t = re.sub(pat, repl, s)
        # two old kernels may become one new one only if they were the same code
        assert renamed.setdefault(t, body) == body, "--rename %s maps different kernels to %s" % (rule, t)
    old = renamed
missing = [s for s in old if s not in new]
differ = [s for s in old if s in new and old[s] != new[s]]
print("old %d symbols, new %d: missing %d, differing %d, added %d" % (
    len(old), len(new), len(missing), len(differ), len([s for s in new if s not in old])))
for s in missing + differ:
    print(("MISSING " if s in missing else "DIFFERS ") + s)
sys.exit(1 if missing or differ else 0)
