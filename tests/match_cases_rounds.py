"""Child process of tests/test_gpu_match_cases.py: the catalogue's level 1-3 cases through the sweeps' rounds.  ZS_FR_RANGE is read
once per process (zs_engine.hip: `static const int env_range`), so every value of it needs a process of its own; ZS_FR_CHUNK is
read per call and is flipped here.  Every case runs alone -- a batch of many short streams takes one workgroup per stream
instead --, the bytes are compared with the oracle's, and one JSON line says what happened."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    import match_cases as mc
    import oracle_binding
    from zlibstream_amd import Engine
    assert os.environ.get("ZS_FR_RANGE") in ("1", "3")
    oracle, engine = oracle_binding.Oracle(), Engine(0)
    names = [n for n in mc.case_names() if mc.case(n)[2] <= 3 and mc.case(n)[4] is None]
    want = {n: oracle.compress(mc.case(n)[1], mc.case(n)[2], mc.case(n)[3]) for n in names}
    out = {"cases": len(names), "bad": [], "calls": 0, "calls_in_rounds": 0, "most_rounds": 0}
    for chunk in ("1024", "2048"):
        os.environ["ZS_FR_CHUNK"] = chunk
        for n in names:
            _, data, level, strategy, _, _ = mc.case(n)
            z = engine.deflate_batch([data], level=level, strategy=strategy)[0]
            rounds = engine.counter("fast_rounds")
            out["calls"] += 1
            out["calls_in_rounds"] += rounds > 0
            out["most_rounds"] = max(out["most_rounds"], rounds)
            if z != want[n]:
                out["bad"].append((chunk, n))
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
