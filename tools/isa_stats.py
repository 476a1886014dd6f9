#!/usr/bin/env python3
"""Compile every kernel unit (crackling_amd/csrc/*.hip) to gfx950 assembly and print, per kernel matching a pattern, its
register / scratch / LDS budget and the counts of the instructions that make up the scan's hot loop (development aid; runs
without a GPU).
    tools/isa_stats.py [name-substring, default k_scan] [--keep /tmp/dir] [--dump DIR]
--dump DIR writes one normalised text per matching kernel: its .amdhsa_* descriptor lines and its body, comments removed and
the .LBB<n>_ labels renumbered to .LBB_ (n counts the functions of the unit).  `diff -r` of the dumps of two trees tells whether
a change of the sources changed any kernel's code."""
import concurrent.futures, pathlib, re, subprocess, sys, tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
opt = lambda name: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None
keep, dump = opt("--keep"), opt("--dump")
pat = next((a for a in sys.argv[1:] if not a.startswith("--") and a not in (keep, dump)), "k_scan")
out_dir = pathlib.Path(keep or tempfile.mkdtemp())
out_dir.mkdir(parents=True, exist_ok=True)


def assembly(src):
    out = out_dir / (src.stem + ".s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950", "-S",
                    "--cuda-device-only", f"-I{ROOT}/include", "-o", str(out), str(src)], check=True, stderr=subprocess.DEVNULL)
    return out.read_text()


units = sorted((ROOT / "crackling_amd/csrc").glob("*.hip"))
with concurrent.futures.ThreadPoolExecutor(max_workers=8) as pool:
    texts = list(pool.map(assembly, units))
demangle = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()
dumped = {}
for s in texts:
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)\.end_amdhsa_kernel", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if pat not in name:
            continue
        get = lambda key: (re.search(rf"\.amdhsa_{key} (\d+)", body) or [None, "?"])[1]
        cnt = lambda p: len(re.findall(p, body))
        print(f"{demangle(name).split('(')[0]}: vgpr {get('next_free_vgpr')} sgpr {get('next_free_sgpr')} "
              f"scratch {get('private_segment_fixed_size')} B lds {get('group_segment_fixed_size')} B | "
              f"v_bitop3 {cnt(r'v_bitop3_b32')} v_xor {cnt(r'v_xor_b32')} v_perm {cnt(r'v_perm_b32')} s_bfe_i32 {cnt(r's_bfe_i32')} "
              f"s_load_x8 {cnt(r's_load_dwordx8')} global_load_x4 {cnt(r'global_load_dwordx4')} ds_read_b128 {cnt(r'ds_read_b128')} "
              f"scratch ops {cnt(r'scratch_(load|store)')} | lines {body.count(chr(10))}")
        if dump:
            lines = (re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0]).rstrip() for l in body.split("\n"))
            text = "\n".join(l for l in lines if l.strip()) + "\n"
            # (the radix kernels of issl_radix.hpp are compiled into two units: the same code both times)
            assert dumped.setdefault(name, text) == text, f"{name}: two units compile it differently"
if dump:
    pathlib.Path(dump).mkdir(parents=True, exist_ok=True)
    for name, text in dumped.items():
        (pathlib.Path(dump) / (name + ".s")).write_text(text)
    print(len(dumped), "kernels dumped to", dump)
if keep:
    print("assembly kept in", out_dir)
