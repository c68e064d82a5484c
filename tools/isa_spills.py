#!/usr/bin/env python3
"""SGPR spills of one kernel, per basic block: compile pt_kernels.hip to gfx950 assembly the way isa_regions.py does and list the
v_readlane_b32 (reload) / v_writelane_b32 (write-back) instructions whose lane selector is a literal — the form the register
allocator's SGPR-to-VGPR-lane spills take; a readlane with a register selector is the program's own — with the source lines their
.loc directives name.  Prints the kernel's next_free_sgpr / next_free_vgpr / scratch / occupancy and a total for the round loop:
the outermost loop that holds the refill's global_load_lds transfers (modes 1 and 2, which have none: the largest outermost loop),
from its header to its back edge, child loops included and counted apart.  Looks at nothing but these two instructions and the
resource lines (and, to find the round loop, at where the global_load_lds transfers stand).
--cold SPEC names the source ranges of the sites a normal round does not pass (the piece switch, seek, the gather step), as
FILE or FILE:A-B joined by commas; the loop's reloads and write-backs whose line lies in none of them are then totalled apart:
the figure per round.  The ranges belong to a revision: give the parent's with the parent's assembly.
usage: tools/isa_spills.py [kernel-substring] [arith 0|1|2] [--asm FILE (an assembly file made elsewhere, e.g. of another revision)] [--cold SPEC]"""
import collections, os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cosc_4397_pathtracing_raytracing_project_amd", "csrc")
args = sys.argv[1:]
asm = None
if "--asm" in args:
    i = args.index("--asm")
    asm = args[i + 1]
    del args[i:i + 2]
cold = []
if "--cold" in args:
    i = args.index("--cold")
    for part in args[i + 1].split(","):
        f, _, r = part.partition(":")
        a, _, b = r.partition("-")
        cold.append((f, int(a) if a else 0, int(b) if b else 1 << 30))
    del args[i:i + 2]
def is_cold(loc):
    f, _, n = loc.partition(":")
    return any(f == cf and a <= int(n or 0) <= b for cf, a, b in cold)
want = args[0] if len(args) > 0 else "k_pathsILNS_6SearchE0ELi3EJEE"
arith = args[1] if len(args) > 1 else "2"
if asm is None:
    asm = os.path.join(ROOT, "build", "scratch", f"pt_regions_{arith}.s")
    os.makedirs(os.path.dirname(asm), exist_ok=True)
    flags = ["-ffp-contract=off"] if arith == "0" else ["-ffp-contract=fast-honor-pragmas"]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", *flags, f"-DPT_ARITH={arith}",
                           "-gline-tables-only", "--cuda-device-only", "-S", "-o", asm, os.path.join(SRC, "pt_kernels.hip")], stderr=subprocess.DEVNULL)
s = open(asm).read()
m = re.search(r"^(_ZN3ptk\S*" + re.escape(want) + r"\S*):(.*?)\n\s*s_endpgm(.*?); COMPUTE_PGM_RSRC2", s, re.S | re.M)
if not m:
    sys.exit(f"no kernel matching {want!r} in {asm}")
name, body, tail = m.group(1), m.group(2), m.group(3)
files = {int(f.group(1)): (f.group(3) or f.group(2)).split("/")[-1] for f in re.finditer(r'\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', s)}
SPILL = re.compile(r"^(v_readlane_b32\s+s\d+,\s*(v\d+)|v_writelane_b32\s+(v\d+),\s*s\d+),\s*(\d+)\s*$")
# the spill registers: the VGPRs that receive SGPRs lane by lane (the program's own readlane with a literal lane reads other registers)
parked = {mm.group(1) for mm in re.finditer(r"^\s*v_writelane_b32\s+(v\d+),\s*s\d+,\s*\d+\s*(?:;.*)?$", body, re.M)}

class Block:
    def __init__(self, label):
        self.label, self.header_of, self.inner, self.parents = label, None, None, []
        self.rd, self.wr, self.instrs, self.lds_dma = collections.Counter(), collections.Counter(), 0, 0

blocks, cur, loc = [], Block("entry"), "?"
blocks.append(cur)
for l in body.splitlines():
    t = l.strip()
    mb = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(.*)", l)
    if mb:
        cur = Block(mb.group(1) or "bb." + mb.group(2))
        blocks.append(cur)
        t = mb.group(3)
    c = re.search(r";\s+in Loop: Header=(BB\d+_\d+) Depth=(\d+)", t)
    if c:
        cur.inner = c.group(1)
    c = re.search(r";\s+Parent Loop (BB\d+_\d+) Depth=(\d+)", t)
    if c:
        cur.parents.append(c.group(1))
    if re.search(r";\s*=>\s*This (Inner )?Loop Header: Depth=(\d+)", t):
        cur.header_of = cur.inner = cur.label
    if mb:
        continue
    ml = re.match(r"\.loc\s+(\d+)\s+(\d+)", t)
    if ml:
        loc = f"{files.get(int(ml.group(1)), '?')}:{ml.group(2)}"
        continue
    if not t or t[0] in ";.":
        continue
    t = t.split(";")[0].strip()
    cur.instrs += 1
    if t.startswith("global_load_lds"):
        cur.lds_dma += 1
    ms = SPILL.match(t)
    if ms and (ms.group(2) or ms.group(3)) in parked:
        (cur.rd if t.startswith("v_readlane") else cur.wr)[loc] += 1
parents = {b.label: b.parents for b in blocks if b.header_of}
def outer(b):  # the outermost loop the block lies in
    if b.inner is None:
        return None
    p = parents.get(b.inner, [])
    return p[0] if p else b.inner
per_loop = collections.defaultdict(lambda: [0, 0])
for b in blocks:
    if outer(b):
        per_loop[outer(b)][0] += b.instrs
        per_loop[outer(b)][1] += b.lds_dma
rnd = max(per_loop, key=lambda h: (per_loop[h][1] > 0, per_loop[h][0])) if per_loop else None
print(f"kernel {name}\narith {arith}, round loop {rnd} ({per_loop[rnd][0] if rnd else 0} instructions)")
for key in ("next_free_sgpr", "next_free_vgpr"):
    mm = re.search(r"\.amdhsa_" + key + r"\s+(\d+)", tail)
    print(f"  {key} {mm.group(1) if mm else '?'}", end="")
for key in ("ScratchSize", "Occupancy", "LDSByteSize"):
    mm = re.search(r"; " + key + r":\s*(\d+)", tail)
    print(f"  {key} {mm.group(1) if mm else '?'}", end="")
print(f"  spill VGPRs {' '.join(sorted(parked)) or 'none'}")
tot = collections.Counter()
for b in blocks:
    nr, nw = sum(b.rd.values()), sum(b.wr.values())
    if not nr and not nw:
        continue
    part = "before/after" if outer(b) != rnd else "round" if b.inner == rnd else "child"
    where = f"round, child loop {b.inner}" if part == "child" else part
    tot[(part, "rd")] += nr
    tot[(part, "wr")] += nw
    if part != "before/after":
        tot[("hot", "rd")] += sum(v for k, v in b.rd.items() if not is_cold(k))
        tot[("hot", "wr")] += sum(v for k, v in b.wr.items() if not is_cold(k))
    lines = collections.Counter()
    for k, v in list(b.rd.items()) + list(b.wr.items()):
        lines[k] += v
    print(f"  {b.label:10s} {where:34s} reloads {nr:3d} write-backs {nw:3d} | " + " ".join(f"{k}x{v}" for k, v in sorted(lines.items())))
print(f"TOTAL round loop, its own blocks: reloads {tot[('round', 'rd')]} write-backs {tot[('round', 'wr')]};"
      f"  its child loops: reloads {tot[('child', 'rd')]} write-backs {tot[('child', 'wr')]};"
      f"  outside the loop: reloads {tot[('before/after', 'rd')]} write-backs {tot[('before/after', 'wr')]}")
if cold:
    print(f"PER ROUND (the loop's blocks and child loops, outside the cold sites): reloads {tot[('hot', 'rd')]} write-backs {tot[('hot', 'wr')]}")
