"""Times a session's load, from texts in host memory to an evaluated session, with and without input
parameters (`validate -i`), for two builds of the library, alternating them run by run:

  N cfg2 templates (30 resources) x the cfg2 rule pack; the parameter file is a small map
  (Parameters.DBPort, as tests/golden/params/input-parameters-dir/db_params.yaml).

    python tools/params_load_measure.py PARENT_LIB NEW_LIB [N] > profiles/params_device_merge_measure.txt

Each library runs in a worker process of its own (GG_LIB); both stay loaded and take turns.  Run 0 of every
mode is the warm-up.  load_s is a host clock around set_params + add_docs_device (add_docs on 16 host threads
when the device loader declines the batch, as a build without the device merge does with parameters) +
upload; eval_ms is the evaluation that follows.  The last `trace` run of the new build prints the loader's
phase marks (GG_LOAD_TRACE), the merge kernel's own time among them, on stderr."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [("db_params.yaml", "Parameters:\n  DBPort:\n    Default: 3306\n")]


def worker():
    sys.path.insert(0, os.path.join(ROOT, "cloudformation-guard_amd"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import guard_amd
    from rulepack import rule_pack
    texts = names = None
    for line in sys.stdin:
        cmd = line.split()
        if cmd[0] == "texts":
            n = int(cmd[1])
            texts = [guard_amd.synth_cfn_doc(i, 30).encode() for i in range(n)]
            names = ["cfg2-%d.json" % i for i in range(n)]
            out = {"docs": n, "text_bytes": sum(map(len, texts))}
        elif cmd[0] == "run":
            if cmd[2] == "trace":
                os.environ["GG_LOAD_TRACE"] = "1"
            s = guard_amd.Session()
            for name, text in rule_pack("cfg2"):
                s.add_rules(text, name)
            t0 = time.perf_counter()
            if cmd[1] == "params":
                s.set_params(PARAMS)
            st = s.add_docs_device(texts, names)
            if st is None:
                s.add_docs(texts, names, threads=16)
            s.upload()
            load_s = time.perf_counter() - t0
            ms = s.eval(1)
            out = {"path": "host" if st is None else "device", "load_s": load_s, "eval_ms": ms[0], "nodes": s.stat(2),
                   "kernel_ms": st and st["kernel_ms"], "GBps": sum(map(len, texts)) / load_s / 1e9}
            s.close()
            os.environ.pop("GG_LOAD_TRACE", None)
        else:
            break
        print(json.dumps(out), flush=True)


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
    for k in procs:
        out["texts_" + k] = ask(k, "texts %d" % n)
    for mode in ("plain", "params"):
        for run in range(4):
            for k in procs:
                out["%s_%s_%d" % (mode, k, run)] = ask(k, "run %s %d" % (mode, run))
    out["params_new_trace"] = ask("new", "run params trace")
    for p in procs.values():
        p.stdin.close()
        p.wait()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    worker() if sys.argv[1:] == ["worker"] else main()
