"""Kernel resources of two builds side by side, in the format of profiles/*_kernel_resources.txt.
   hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -c -Rpass-analysis=kernel-resource-usage \
         -o /dev/null media_amd/csrc/mi355x_h264.hip 2> remarks.txt      (once in the parent's tree, once in the new one)
   python tools/kernel_resources.py parent_remarks.txt new_remarks.txt [OLD=NEW ...] > profiles/NAME_kernel_resources.txt
OLD=NEW: the parent's kernel OLD is the new build's kernel NEW (a kernel that became a template, say): compared as one row."""
import re
import subprocess
import sys

KEYS = (("VGPRs", "VGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
        ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    out, order, cur = {}, [], None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            order.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out, order


def demangle(names):
    r = subprocess.run(["c++filt", "-p"], input="\n".join(names), capture_output=True, text=True)
    return dict(zip(names, [re.sub(r"^void ", "", x) for x in r.stdout.split("\n")])) if r.returncode == 0 else {n: n for n in names}


def main():
    old, _ = parse(sys.argv[1])
    new, order = parse(sys.argv[2])
    renamed = dict(a.split("=", 1) for a in sys.argv[3:])
    if renamed:   # by demangled name: the parent's entry moves under the new build's mangled name
        was = demangle(list(old))
        now = {v: k for k, v in demangle(order).items()}
        for o, n in renamed.items():
            key = [k for k, v in was.items() if v == o]
            assert len(key) == 1 and n in now, (o, n)
            old[now[n]] = old.pop(key[0])
    names = demangle(order + [n for n in old if n not in new])
    for o, n in renamed.items():
        names[now[n]] = "%s (parent: %s)" % (n, o)
    print("kernel-resource-usage remarks, hipcc -O3 --offload-arch=gfx950, parent / new build (p/n); * = differs; - = not in that build")
    print("kernel | " + " | ".join(k[1] + " p/n" for k in KEYS))
    differ = added = 0
    for n in order + [n for n in old if n not in new]:
        a, b = old.get(n), new.get(n)
        cells = ["%s/%s" % (a[k[0]] if a else "-", b[k[0]] if b else "-") for k in KEYS]
        star = ""
        if a and b and any(a[k[0]] != b[k[0]] for k in KEYS):
            star, differ = " *", differ + 1
        if not a:
            added += 1
        print("%s | %s%s" % (names[n], " | ".join(cells), star))
    both = sum(1 for n in new if n in old)
    print("%d kernels in both builds, %d rows differ; %d kernels are new, %d left" % (both, differ, added, sum(1 for n in old if n not in new)))


if __name__ == "__main__":
    main()
