"""Sensitivity of tests/test_nee_path.py: seven changes to
a scratch copy of csrc/rt_cpu.cpp's path loop, each built into a scratch
libbwrt.so (the tree's other objects, untouched) and run against the CPU-twin
tests through BWRT_LIB.  CPU only: no kernel text is mutated and nothing here
touches a GPU.  Every mutant must fail at least one test.

  python tools/nee_path_sensitivity.py [scratch directory]

Prints one line per mutant: how many of the CPU-twin cases fail, and the first.
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "bwidman-raytracer_amd")
SRC = os.path.join(PKG, "csrc", "rt_cpu.cpp")

DIFFUSE = "            scatter = random_direction(rs, n);  // brdf = 4 * albedo\n"
END_OF_BRANCH = "                }\n            }\n        }\n        rec_code[depth] = code;\n"

# name -> [(old text, new text)]; every old text occurs exactly once
MUTANTS = {
    "suppression asked with the new hit's point": [
        ("light_suppressed<SHAPES>(K, N, o, nee_prim, id)", "light_suppressed<SHAPES>(K, N, P, nee_prim, id)")],
    "nee_prim kept from one inner path to the next": [
        ("template <bool NEE, int PICK, int SHAPES>\nf3 trace_path(", "static thread_local int g_nee_prim = -1;\n"
         "template <bool NEE, int PICK, int SHAPES>\nf3 trace_path("),
        ("    [[maybe_unused]] int nee_prim = -1;", "    int& nee_prim = g_nee_prim;"),
        ("        f3 L = trace_path<NEE, PICK, SHAPES>(K, N, rs, cam, dcam);\n",
         "        g_nee_prim = -1;\n        f3 L = trace_path<NEE, PICK, SHAPES>(K, N, rs, cam, dcam);\n")],
    "depth + 1 < max_bounces": [("depth + 1 <= K.max_bounces &&", "depth + 1 < K.max_bounces &&")],
    "visible on any hit": [("if (ids == s.prim) aux |= RT_NEE_VISIBLE;", "if (ids >= 0) aux |= RT_NEE_VISIBLE;")],
    "the kind-0 test dropped": [("N.n_lights > 0 && kind) {", "N.n_lights > 0) {")],
    "the drop on the level's own emission": [
        ("nee_prim, id)) aux = RT_NEE_DROP;", "nee_prim, id)) rec_aux[depth - 1] |= RT_NEE_DROP;")],
    "the NEE draws before random_direction's": [
        (DIFFUSE, ""),
        (END_OF_BRANCH, END_OF_BRANCH.replace("            }\n        }\n", "            }\n" + DIFFUSE + "        }\n"))],
}


def sh(cmd, **kw):
    return subprocess.run(cmd, cwd=PKG, text=True, capture_output=True, **kw)


def make_vars():
    """HIPCC and the flag lines of the Makefile, as make expands them"""
    db = sh(["make", "-pn", "lib"]).stdout
    out = {}
    for name in ("HIPCC", "CPUFLAGS", "HIPFLAGS", "LDFLAGS", "OBJS", "TUNE", "ROCM", "ARCH"):
        m = re.search(rf"^{name} [:?]?= (.*)$", db, re.M)
        out[name] = m.group(1) if m else ""
    for _ in range(3):
        for k in out:
            out[k] = re.sub(r"\$\((\w+)\)", lambda m: out.get(m.group(1), ""), out[k])
    return out


def main():
    scratch = sys.argv[1] if len(sys.argv) > 1 else tempfile.mkdtemp(prefix="nee_path_mutants")
    v = make_vars()
    text = open(SRC).read()
    objs = [o for o in v["OBJS"].split() if not o.endswith("rt_cpu.o")]
    assert all(os.path.exists(os.path.join(PKG, o)) for o in objs), "build the tree first"
    failed_all = True
    for i, (name, edits) in enumerate(MUTANTS.items(), 1):
        d = os.path.join(scratch, f"m{i}")
        os.makedirs(d, exist_ok=True)
        t = text
        for old, new in edits:
            assert t.count(old) == 1, (name, old)
            t = t.replace(old, new)
        src, obj, lib = os.path.join(d, "rt_cpu.cpp"), os.path.join(d, "rt_cpu.o"), os.path.join(d, "libbwrt.so")
        open(src, "w").write(t)
        r = sh([v["HIPCC"], *v["CPUFLAGS"].split(), "-Icsrc", "-c", "-o", obj, src])
        assert r.returncode == 0, r.stderr
        r = sh([v["HIPCC"], *v["HIPFLAGS"].split(), *v["LDFLAGS"].split(), "-o", lib, *objs, obj])
        assert r.returncode == 0, r.stderr
        env = dict(os.environ, BWRT_LIB=lib)
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(REPO, "tests", "test_nee_path.py"), "-q", "-k", "cpu_twin",
                            "-p", "no:cacheprovider", "-rf"], cwd=REPO, env=env, text=True, capture_output=True)
        failed = re.findall(r"^FAILED \S+::(\S+)", r.stdout, re.M)
        total = re.search(r"(\d+) passed", r.stdout)
        failed_all &= bool(failed)
        print(f"{i}. {name}: {len(failed)} of {len(failed) + (int(total.group(1)) if total else 0)} fail"
              + (f", first {failed[0]}" if failed else "  <-- NOT DETECTED"), flush=True)
        for f in failed:
            print(f"     {f}")
    return 0 if failed_all else 1


if __name__ == "__main__":
    sys.exit(main())
