"""One line per gfx950 kernel of each given .hip file: symbol, a hash of its instruction stream, VGPR / AGPR / SGPR counts, fixed LDS bytes
and private-segment (spill) bytes.  A refactor that must not move code is checked by running this on both commits and `diff`ing the output.
The files are compiled with the product build's compiler and flags (-save-temps).  The hash covers the instruction and label lines of the
kernel's function with comments and directives (debug and other; alignment stays) dropped and the `.LBB<n>_` label prefixes normalised, so
the order of the functions in the file does not matter.  Counts and sizes come from the notes, checked against the kernel descriptor.
    python tools/isa_fingerprint.py file.hip [file.hip ...]"""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from walkgpt_amd import _build  # noqa: E402  (the flags the product objects are built with)


def fingerprint(src):
    """[(symbol, hash, vgprs, agprs, sgprs, lds bytes, private bytes)] of the kernels of one .hip file, sorted by symbol."""
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([_build.HIPCC] + _build.FLAGS + ["-save-temps=obj", "-c", os.path.abspath(src), "-o", os.path.join(tmp, "x.o")],
                           capture_output=True, text=True, cwd=tmp)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed for %s:\n%s" % (src, r.stderr))
        text = open(os.path.join(tmp, [f for f in os.listdir(tmp) if f.endswith("gfx950.s")][0])).read()
    # the notes: one YAML map per kernel, `  - ` opens it, its keys are indented by four blanks (its arguments' by more)
    notes = {}
    for entry in re.split(r"^  - ", text[text.index("amdhsa.kernels:"):], flags=re.M)[1:]:
        kv = dict(re.findall(r"^(?:    )?\.(\w+): +(\S+)$", entry, flags=re.M))
        if "name" in kv:   # (the version list behind the kernels splits the same way)
            notes[kv["name"]] = kv
    out = []
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M):
        body = text[text.index("\n%s:" % sym):]
        body = body[:body.index("\n\t.section")]
        h = hashlib.sha256()
        for ln in body.split("\n")[1:]:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())
            if ln and (ln[0] != "." or ln.startswith((".LBB_", ".p2align"))):   # instructions, block labels, alignment
                h.update((" ".join(ln.split()) + "\n").encode())
        desc = text[text.index(".amdhsa_kernel %s\n" % sym):]
        desc = dict(re.findall(r"^\s*\.amdhsa_(\w+) (\S+)$", desc[:desc.index(".end_amdhsa_kernel")], flags=re.M))
        n = notes[sym]
        assert desc["group_segment_fixed_size"] == n["group_segment_fixed_size"] and desc["private_segment_fixed_size"] == n["private_segment_fixed_size"], sym
        out.append((sym, h.hexdigest()[:16], int(n["vgpr_count"]), int(n["agpr_count"]), int(n["sgpr_count"]),
                    int(n["group_segment_fixed_size"]), int(n["private_segment_fixed_size"])))
    return sorted(out)


if __name__ == "__main__":
    for path in sys.argv[1:]:
        for k in fingerprint(path):
            print("%s %s vgpr=%d agpr=%d sgpr=%d lds=%d private=%d" % k)
