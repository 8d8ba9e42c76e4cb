"""Times the counted device report entries (Session.report_<format>_device: size pass, write pass, copy-out,
host-written documents) for two builds of the library, alternating them run by run, on two corpora:

  floats -- N cfg2 templates (30 resources) x the cfg2 rule pack, device-loaded; in every second template each
            AWS::EC2::Volume's "Size" is a float (123 -> 123.5).  ebs-volume-encryption.guard reports it as
            the compared value of `Properties.Size <= 256` and inside the Properties struct that
            `Properties.Encrypted exists` traversed to;
  plain  -- the same templates unmodified (no float anywhere).

    python tools/float_report_measure.py PARENT_LIB NEW_LIB [N] > profiles/float_device_report_measure.txt

Each library runs in a worker process of its own (GG_LIB); both stay loaded and take turns.  Run 0 of every
(corpus, format) is the warm-up.  wall_s is a host clock around the call, which ends after the copy to host
memory; the *_ms fields are the library's own stage times."""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def worker():
    sys.path.insert(0, os.path.join(ROOT, "cloudformation-guard_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import guard_amd
    from rulepack import rule_pack
    s = None
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == "load":
            if s:
                s.close()
            n, floats = int(cmd[1]), cmd[2] == "floats"
            texts = [guard_amd.synth_cfn_doc(i, 30).encode() for i in range(n)]
            if floats:
                texts = [re.sub(rb'"Size":(\d+)', rb'"Size":\1.5', t) if i % 2 else t for i, t in enumerate(texts)]
            s = guard_amd.Session()
            for name, text in rule_pack("cfg2"):
                s.add_rules(text, name)
            st = s.add_docs_device(texts, ["cfg2-%d.json" % i for i in range(n)])
            ms = s.eval(1)
            out = {"docs": n, "text_bytes": sum(map(len, texts)), "refused_docs": st["refused_docs"], "eval_ms": ms[0]}
        elif cmd[0] == "run":
            t0 = time.perf_counter()
            nbytes, code, out = getattr(s, "report_%s_device" % cmd[1])()
            dt = time.perf_counter() - t0
            out.update(bytes=nbytes, code=code, wall_s=dt, GBps=nbytes / dt / 1e9)
        else:
            break
        print(json.dumps(out), flush=True)
    if s:
        s.close()


def main():
    libs = {"parent": os.path.abspath(sys.argv[1]), "new": os.path.abspath(sys.argv[2])}
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    procs = {k: subprocess.Popen([sys.executable, os.path.abspath(__file__), "worker"], env=dict(os.environ, GG_LIB=v),
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for k, v in libs.items()}

    def ask(k, cmd):
        procs[k].stdin.write(cmd + "\n")
        procs[k].stdin.flush()
        line = procs[k].stdout.readline()
        while line and not line.startswith("{"):   # (anything else a library prints)
            line = procs[k].stdout.readline()
        if not line:   # the worker ended (an error, a fault): nothing more is started
            for p in procs.values():
                p.kill()
            raise SystemExit("worker %r ended at %r" % (k, cmd))
        print(k, cmd, line.strip(), file=sys.stderr, flush=True)
        return json.loads(line)

    out = {"docs": n, "rules_files": 7}
    for corpus, formats in (("floats", ("json", "yaml", "sarif", "junit")), ("plain", ("json", "yaml"))):
        for k in procs:
            out["%s_load_%s" % (corpus, k)] = ask(k, "load %d %s" % (n, corpus))
        for fmt in formats:
            for run in range(4):
                for k in procs:
                    out["%s_%s_%s_%d" % (corpus, fmt, k, run)] = ask(k, "run " + fmt)
    for p in procs.values():
        p.stdin.close()
        p.wait()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    worker() if sys.argv[1:] == ["worker"] else main()
