"""Are the kernels of one build, instruction for instruction, the kernels of another?

    hipcc --offload-arch=gfx950 -O3 -std=c++17 [the file's flags of build.py] --cuda-device-only -S -x hip FILE -o a.s   (commit A)
    ... the same at commit B -> b.s
    python tools/compare_kernel_asm.py a.s b.s

Per symbol of a.s: the instruction lines of its body (comments, directives and blank lines dropped; basic-block labels
.LBB<function>_<block> renumbered without the function index, which shifts whenever a kernel is added in front) against the
body of the same symbol in b.s.  Prints the symbols that differ or are missing and the symbols only b.s has; exit status 1
if any symbol of a.s changed.  The use: a pull request that adds template instantiations to dec_kernels.hip shows that the
existing ones came out unchanged."""
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        if line.lstrip().startswith(".amdgpu_metadata"):   # the YAML note behind the code: not instructions
            break
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is not None:
            t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", line.split(";")[0].strip())
            if t and not t.startswith("."):
                cur.append(t)
    return {k: v for k, v in out.items() if v and not k.startswith("__hip_cuid")}


def main(a_path, b_path):
    a, b = functions(a_path), functions(b_path)
    changed = 0
    for name, body in a.items():
        if name not in b:
            print("missing:", name)
            changed += 1
        elif body != b[name]:
            print("differs: %s (%d -> %d instructions)" % (name, len(body), len(b[name])))
            changed += 1
    new = sorted(set(b) - set(a))
    print("%d symbols in %s: %d identical in %s, %d changed or missing; %d symbols only in %s"
          % (len(a), a_path, len(a) - changed, b_path, changed, len(new), b_path))
    for name in new:
        print("new:", name)
    return 1 if changed else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
