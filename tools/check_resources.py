"""Register / scratch report of every kernel of libmmx_hip.so (hipcc -Rpass-analysis=kernel-resource-usage over csrc/*.hip) and
the build's spill gate: the kernels the engines' DEFAULTS launch must have ScratchSize 0 (`make -C minimax-speech_amd/csrc check`).

    python tools/check_resources.py [file.hip ...] [--all]      (--all: print every kernel, not only the gated / spilling ones)
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimax-speech_amd", "csrc")
FLAGS = "-O3 --offload-arch=gfx950 -fPIC -std=c++20 -Wno-unused-result -Wno-pass-failed -Rpass-analysis=kernel-resource-usage".split()
# demangled-name prefixes of the kernels the default configurations launch (mmx/flow.py, mmx/llm.py, mmx/dac.py tile rules); the
# est_tail / est_resnet forms are those the static_asserts under tail_select / resnet_select in csrc/fused.hip pin to the defaults
GATED = [
    "est_tail_kernel<unsigned short, 64, 2, 8, 1, 1, 2, false>",      # bf16 build, 64-row tiles
    "est_tail_kernel<unsigned short, 32, 8, 8, 1, 1, 2, false>",      # bf16 build, 32-row tiles
    "est_tail_kernel<unsigned short, 16, 8, 4, 1, 1, 4, false>",      # bf16 build, 16-row tiles
    "est_tail_kernel<unsigned short, 64, 2, 8, 2, 1, 2, false>",         # split build, 64-row tiles (K-halved attention tile)
    "est_tail_kernel<unsigned short, 32, 2, 8, 2, 1, 4, false>",         # split build
    "est_tail_kernel<unsigned short, 16, 4, 8, 2, 1, 4, false>",      # split build, 16-row tiles (8 waves)
    "est_tail_kernel<unsigned short, 64, 2, 8, 2, 1, 2, true>", "est_tail_kernel<unsigned short, 32, 2, 8, 2, 1, 4, true>",       # split build, weight planes
    "est_tail_kernel<unsigned short, 16, 4, 8, 2, 1, 4, true>",
    "est_resnet_kernel<unsigned short, 64, 2, 8, 1, false>", "est_resnet_kernel<unsigned short, 32, 4, 8, 1, false>",
    "est_resnet_kernel<unsigned short, 32, 2, 4, 2, false>", "est_resnet_kernel<unsigned short, 32, 4, 4, 2, false>",
    "est_resnet_kernel<unsigned short, 32, 4, 8, 2, false>", "est_resnet_kernel<unsigned short, 32, 4, 8, 2, true>",   # split build, 8 waves (cin = 256)
    "est_resnet_kernel<unsigned short, 32, 2, 4, 2, true>", "est_resnet_kernel<unsigned short, 32, 4, 4, 2, true>",
    "skinny3_kernel", "decode_attn_kernel", "sample_step_kernel", "attn_flash_kernel", "attn_flash_x_kernel", "attn_relpos",
    "dac_ru_kernel", "gemm_win_kernel", "logmel_kernel", "pool_rows_kernel", "logmel_w_finish", "s3_rope_fsmn_kernel",
    "fsq_encode_kernel", "rownorm_kernel", "resample_sinc_kernel", "kweight_kernel", "kweight_carry_kernel", "loudness_gate_kernel",
    "scale_rows_kernel", "spec_dist_kernel", "spec_finish_kernel", "wave_sums_kernel", "wave_finish_kernel",
    "gate_stft_kernel", "gate_thresh_kernel", "gate_synth_kernel", "gate_ola_kernel",
    "stoi_energy_kernel", "stoi_scan_kernel", "stoi_bands_kernel", "stoi_score_kernel", "stoi_finish_kernel",
    "ir_prepare_kernel", "ir_table_kernel", "fir_rows_kernel", "row_absmax_kernel", "mix_rows_kernel",
    "pad_edge_kernel", "row_select_kernel", "clip_rows_kernel", "quantize_rows_kernel",
]


# register ceilings (VGPRs + AGPRs per wave) that a design decision rests on, and the dynamic LDS the launcher asks for (bytes; the
# compiler does not see it: read from the launcher's source)
#   attn_flash_x_kernel<1, true, 8>: the form launched beside the LM decode loop.  Two of its waves per SIMD must leave 224 registers
#   for decode workgroups (2 x 96-112): (512 - 224) / 2 = 144.  Every form of the kernel holds 64 KB of LDS (K and V^T, hi + lo planes,
#   double buffered; P stays in registers), so two 128-query workgroups, or one and a decode workgroup, fit in a CU's 160 KB.
REG_MAX = {"attn_flash_x_kernel<1, true, 8>": 144}
LDS_EXPECT = {"attention_x.hip": ("launch_flash_x", r"const size_t lds = \(size_t\)8 \* 64 \* 128;", 64 * 1024)}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return out.strip().split("\n")


def report(path):
    with tempfile.NamedTemporaryFile(suffix=".o") as tmp:
        err = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "-c", path, "-o", tmp.name], capture_output=True, text=True, cwd=CSRC).stderr
    rows, cur = [], None
    for line in err.split("\n"):
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|TotalSGPRs): (\S+)", line)
        if not m:
            continue
        k, v = m.groups()
        if k == "Function Name":
            cur = {"name": v}
            rows.append(cur)
        else:
            cur[k.split(" ")[0] + ("_spill" if "Spill" in k else "")] = int(v)
    names = demangle([r["name"] for r in rows])
    for r, n in zip(rows, names):
        n = re.sub(r"\(anonymous namespace\)::|^void ", "", n)
        r["name"] = n.split("(")[0] if "<" not in n else n[:n.rindex(">") + 1]
    return rows


def main():
    files = [a for a in sys.argv[1:] if a.endswith(".hip")] or sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    show_all = "--all" in sys.argv
    bad, over = [], []
    for f in files:
        for r in report(os.path.join(CSRC, f)):
            gated = any(g in r["name"] for g in GATED)
            spills = r.get("ScratchSize", 0) > 0
            if show_all or spills or gated:
                print(f"{f:16s} {r['name'][:96]:96s} vgpr {r.get('VGPRs', 0):3d} agpr {r.get('AGPRs', 0):3d} scratch {r.get('ScratchSize', 0):4d} "
                      f"occ {r.get('Occupancy', 0)}{'  GATED' if gated else ''}{'  SPILLS' if spills else ''}")
            if gated and spills:
                bad.append(r["name"])
            cap = REG_MAX.get(r["name"])
            if cap is not None and r.get("VGPRs", 0) + r.get("AGPRs", 0) > cap:
                over.append(f"{r['name']}: {r.get('VGPRs', 0) + r.get('AGPRs', 0)} registers > {cap}")
        if f in LDS_EXPECT:
            fn, pat, nbytes = LDS_EXPECT[f]
            src = open(os.path.join(CSRC, f)).read()
            if not re.search(pat, src[src.index(fn):]):
                over.append(f"{f}: {fn} no longer asks for {nbytes} bytes of LDS")
    if bad:
        print("\nspilling kernels on a default path:\n  " + "\n  ".join(bad))
        sys.exit(1)
    if over:
        print("\nresource expectations not met:\n  " + "\n  ".join(over))
        sys.exit(1)
    print("\nno gated default-path kernel spills; register ceilings and LDS sizes as expected")


if __name__ == "__main__":
    main()
