"""Wait audit of a kernel in a `hipcc -S` listing: for every `s_waitcnt vmcnt(N)`, its line in
the kernel's listing, whether a backward branch encloses it, and the vector-memory instructions
issued since the previous vmcnt wait.
    python scripts/wait_audit.py LISTING.s 'k_nodes<128, 1, 0, false>' [FIRST_LINE LAST_LINE]"""
import re
import subprocess
import sys
from collections import Counter


def demangle(name):
    return subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()


def kernels(path):
    """Mangled name -> body lines of every function of the listing."""
    cur, body, out = None, [], {}
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and cur is None:
            cur, body = m.group(1), []
        elif cur is not None:
            if ln.startswith(".Lfunc_end"):
                out[cur] = body
                cur = None
            else:
                body.append(ln.rstrip("\n"))
    return out


def audit(body):
    """(line, N, in a loop, instructions since the previous wait) of every vmcnt wait."""
    labels = {}
    for i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, ln in enumerate(body):
        m = re.search(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and labels.get(m.group(1), i + 1) <= i:
            loops.append((labels[m.group(1)], i))
    since, rows = [], []
    for i, ln in enumerate(body):
        t = ln.strip()
        if re.match(r"(global|buffer|flat|scratch)_(load|store|atomic)", t):
            since.append(t.split()[0])
        m = re.search(r"s_waitcnt.*vmcnt\((\d+)\)", t)
        if m:
            rows.append((i, int(m.group(1)), any(a <= i <= b for a, b in loops), since))
            since = []
    return rows


if __name__ == "__main__":
    path, pat = sys.argv[1], sys.argv[2]
    lo, hi = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, 1 << 30)
    for name, body in kernels(path).items():
        d = demangle(name)
        if pat not in d:
            continue
        print("==", d.split("(")[0], "lines", len(body))
        for i, n, in_loop, since in audit(body):
            if lo <= i <= hi:
                issued = ", ".join(f"{v}x {k}" for k, v in Counter(since).items())
                print(f"  line {i:6d} vmcnt({n}) {'loop' if in_loop else '    '}  since: {issued}")
