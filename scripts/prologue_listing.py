"""Read the prologues of the split-fp32 kernels off a gfx950 assembly listing (no GPU needed).

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -Isgam_neurips22_amd/csrc -Iinclude \
          sgam_neurips22_amd/csrc/conv_f32x.hip -o conv_f32x.s
    python scripts/prologue_listing.py conv_f32x.s [--match halo2]

Per kernel, one row:
  batches   groups of s_load separated by a wait (s_waitcnt lgkmcnt) in front of the first vector load: each is one dependent
            trip to memory for the kernel arguments
  first     the vector loads up to the first MFMA in issue order, run-length coded: g = global_load (GroupNorm parameters, combine
            operands), b<n> = buffer_load through the n-th distinct resource in order of appearance (halo / weights)
  waits     the vmcnt waits between the first vector load and the first MFMA (for a kernel without MFMA: up to the first store)
  br        conditional branches between the first vector load and the first MFMA
  vgpr / agpr / scratch / sgpr / occ   from the kernel's "Kernel info" comment; lane-moves = v_writelane / v_readlane in the whole
            kernel (scalar values parked in vector lanes; the epilogue's shuffles count too, so compare against the parent)
"""
import argparse
import re
import subprocess


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.SubprocessError):
        return {n: n for n in names}


def kernels(text):
    """name -> (instruction lines, metadata dict)"""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?); WaveLimiterHint", text, re.S | re.M):
        name, body, tail = m.group(1), m.group(2), m.group(3)
        md = {k: int(v) for k, v in re.findall(r"; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy): (\d+)", tail)}
        md["spill"] = len(re.findall(r"v_writelane_b32|v_readlane_b32", body))
        ins = [ln.strip() for ln in body.split("\n") if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        out[name] = (ins, md)
    return out


def is_vload(i):
    return i.startswith(("buffer_load", "global_load", "flat_load", "scratch_load"))


def prologue(ins):
    first = next((k for k, i in enumerate(ins) if is_vload(i)), len(ins))
    batches, pending = 0, False
    for i in ins[:first]:
        if i.startswith(("s_load", "s_buffer_load")):
            pending = True
        elif i.startswith("s_waitcnt") and "lgkmcnt" in i and pending:
            batches, pending = batches + 1, False
    batches += pending
    end = next((k for k, i in enumerate(ins) if i.startswith("v_mfma")), None)
    if end is None:
        end = next((k for k, i in enumerate(ins) if i.startswith(("global_store", "buffer_store"))), len(ins))
    seq, waits, rsrc, br = [], [], {}, 0
    for i in ins[first:end]:
        if i.startswith("global_load") or i.startswith("flat_load"):
            seq.append("g")
        elif i.startswith("buffer_load"):
            r = re.search(r"(s\[\d+:\d+\])", i)
            seq.append("b%d" % rsrc.setdefault(r.group(1) if r else "?", len(rsrc)))
        elif i.startswith("s_waitcnt") and "vmcnt" in i:
            waits.append(int(re.search(r"vmcnt\((\d+)\)", i).group(1)))
            seq.append("|")
        elif i.startswith("s_cbranch"):
            br += 1
    rl, prev, n = [], None, 0
    for t in seq + [None]:
        if t == prev:
            n += 1
            continue
        if prev is not None:
            rl.append(prev if prev == "|" else f"{prev}x{n}")
        prev, n = t, 1
    return batches, " ".join(rl), waits, br, first


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("listing")
    ap.add_argument("--match", default="f32x", help="substring of the demangled kernel name")
    args = ap.parse_args()
    ks = kernels(open(args.listing).read())
    names = demangle(list(ks))
    for mangled, (ins, md) in ks.items():
        name = re.sub(r"^void \(anonymous namespace\)::|\(\(anonymous namespace\)::XParams\)$", "", names[mangled])
        if args.match not in name:
            continue
        batches, seq, waits, br, first = prologue(ins)
        print(f"{name}\n    batches {batches}  (first vector load is instruction {first})  branches {br}\n    first   {seq}\n    waits   {waits}\n"
              f"    vgpr {md.get('NumVgprs')} agpr {md.get('NumAgprs')} scratch {md.get('ScratchSize')} "
              f"sgpr {md.get('TotalNumSgprs')} lane-moves {md.get('spill')} occ {md.get('Occupancy')}")


if __name__ == "__main__":
    main()
