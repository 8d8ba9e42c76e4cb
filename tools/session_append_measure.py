"""Times a device append (gg_session_add_docs_device on a session that holds documents) on one MI355X:
(a) against gg_session_add_docs with 16 host threads on the same second batch into the same session,
(b) against a one-shot device load of both halves, with the second half loaded into an empty session as
the share that is not seeding or growth.  Prints one JSON document; every answer also goes to stderr as
it comes.  Usage: session_append_measure.py [docs per half] [repeats] [upload: time the uploads instead]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cloudformation-guard_amd"))
import guard_amd  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 262144
REPEATS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RES = 50
L = guard_amd.lib()


def texts(first, n):
    buf = ctypes.create_string_buffer(1 << 20)
    out = []
    for i in range(first, first + n):
        k = L.gg_synth_cfn_doc(i, RES, buf, len(buf))
        out.append(buf.raw[:k])
    return out


def first_half():
    s = guard_amd.Session()
    assert s.add_synthetic_device(0, N, RES, 16) is not None
    return s


def answer(what, wall, st, s):
    r = {"wall_s": wall, "kernel_ms": st and st["kernel_ms"], "h2d_ms": st and st["h2d_ms"], "d2h_ms": st and st["d2h_ms"],
         "added_strings": st and st["distinct_strings"], "added_pool_bytes": st and st["pool_bytes"],
         "ndocs": s.stat(s.STAT["ndocs"]), "nodes": s.stat(s.STAT["nodes"]), "pool_bytes": s.stat(s.STAT["bytes"])}
    print(what, json.dumps(r), file=sys.stderr, flush=True)
    s.close()
    return r


def synthetic(s, first, n):   # wall without the host's text generation, which the entry times itself
    t0 = time.perf_counter()
    st = s.add_synthetic_device(first, n, RES, 16)
    return time.perf_counter() - t0 - st["gen_ms"] / 1e3, st


def uploads():
    """the upload after an append (packs the new range) against the first upload of as many documents"""
    out = {}
    for r in range(-1, REPEATS):
        tag = "warmup" if r < 0 else str(r)
        for what, halves in (("upload_after_append_", 2), ("upload_one_shot_", 1)):
            s = guard_amd.Session()
            s.add_rules(RULE, "ebs.guard")
            ups = []
            for h in range(halves):
                assert s.add_synthetic_device(h * N, N * (3 - halves), RES, 16) is not None
                t0 = time.perf_counter()
                s.upload()
                ups.append(time.perf_counter() - t0)
            out[what + tag] = {"upload_s": ups, "ndocs": s.stat(s.STAT["ndocs"])}
            print(what + tag, json.dumps(out[what + tag]), file=sys.stderr, flush=True)
            s.close()
    print(json.dumps(out, indent=1))


RULE = "rule EBS_VOLUMES_ENCRYPTED {\n    AWS::EC2::Volume {\n        Properties.Encrypted == true\n    }\n}\n"


def main():
    if len(sys.argv) > 3 and sys.argv[3] == "upload":
        return uploads()
    second = texts(N, N)
    T = (ctypes.c_char_p * N)(*second)
    Ls = (ctypes.c_size_t * N)(*[len(t) for t in second])
    Nm = (ctypes.c_char_p * N)(*[b"synthetic-%d.json" % (N + i) for i in range(N)])
    out = {"docs_per_half": N, "resources": RES, "second_half_text_bytes": sum(len(t) for t in second)}
    print("texts", json.dumps(out), file=sys.stderr, flush=True)
    for r in range(-1, REPEATS):   # -1: warm-up (code objects, block cache, pinned staging)
        tag = "warmup" if r < 0 else str(r)
        s = first_half()
        st = (ctypes.c_double * len(guard_amd.LOAD_STATS))()
        err = guard_amd.ExternError()
        t0 = time.perf_counter()
        rc = L.gg_session_add_docs_device(s.s, T, Ls, Nm, N, st, ctypes.byref(err))
        wall = time.perf_counter() - t0
        assert rc == 0, rc
        out["append_device_" + tag] = answer("append_device " + tag, wall, dict(zip(guard_amd.LOAD_STATS, list(st))), s)
        s = first_half()
        err = guard_amd.ExternError()
        t0 = time.perf_counter()
        L.gg_session_add_docs(s.s, T, Ls, Nm, N, 0, 16, ctypes.byref(err))
        wall = time.perf_counter() - t0
        assert err.code == 0, err.code
        out["append_host16_" + tag] = answer("append_host16 " + tag, wall, None, s)
        s = first_half()
        wall, st = synthetic(s, N, N)
        out["append_synthetic_" + tag] = answer("append_synthetic " + tag, wall, st, s)
        s = guard_amd.Session()
        wall, st = synthetic(s, N, N)
        out["second_half_alone_" + tag] = answer("second_half_alone " + tag, wall, st, s)
        s = guard_amd.Session()
        wall, st = synthetic(s, 0, 2 * N)
        out["one_shot_" + tag] = answer("one_shot " + tag, wall, st, s)
    s = first_half()
    os.environ["GG_LOAD_TRACE"] = "1"   # the loader's phase marks of one more append, on stderr
    print("traced append follows", file=sys.stderr, flush=True)
    wall, st = synthetic(s, N, N)
    out["append_synthetic_trace"] = answer("append_synthetic trace", wall, st, s)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
