#!/usr/bin/env python3
"""Launch signatures of Generator.forward: what a change to generator.py must leave alone.

    generator_launches.py --out FILE        run every case on cuda:0 and write its signatures (one process, one tree)
    generator_launches.py --compare A B     per-case call counts of two such files and whether they are equal (exit 1 if not)

The signature of one forward is every C call in order with all its arguments, plus every torch.cuda.Event.record / Stream.wait_event /
Stream.wait_stream, with each pointer, stream and event replaced by the ordinal of its first appearance in that forward: equal
signatures mean the same launches on the same buffers, streams and events in the same order.  Size queries (*_scratch_bytes,
dispu_linear_plan) launch nothing and are left out.  Each case is recorded twice on one Generator: cold (the workspace and the lazy
buffers are allocated on the way) and warm.  The script touches only attributes every version of the Generator has, so the same file
runs in a checkout of an older commit; compare the two outputs with --compare."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CASES = [   # (name, dtype, (B, N), attributes set on the Generator)
    ("f32 (32, 256)", "f32", (32, 256), {}),
    ("f32 (3, 256)", "f32", (3, 256), {}),
    ("f32 (2, 250)", "f32", (2, 250), {}),
    ("f32 (1, 288)", "f32", (1, 288), {}),
    ("f32 (2, 1024)", "f32", (2, 1024), {}),
    ("f32 (3, 256) fused_local off", "f32", (3, 256), {"fused_local": False}),
    ("f32 (3, 256) fused_attention off", "f32", (3, 256), {"fused_attention": False}),
    ("f32 (3, 256) fused_project off", "f32", (3, 256), {"fused_project": False}),
    ("f32 (3, 256) fused_heads off", "f32", (3, 256), {"fused_heads": False}),
    ("f32 (3, 256) chain_inputs off", "f32", (3, 256), {"chain_inputs": False}),
    ("f32 (3, 256) branches off", "f32", (3, 256), {"branches": False}),
    ("f32 (3, 256) split_bf16 on", "f32", (3, 256), {"split_bf16": True}),
    ("f32 (3, 256) keep_intermediates on", "f32", (3, 256), {"keep_intermediates": True}),
    ("f32 (3, 256) fine_out set", "f32", (3, 256), {"fine_out": (3, 1024, 3)}),
    ("bf16 (32, 256)", "bf16", (32, 256), {}),
    ("bf16 (2, 250)", "bf16", (2, 250), {}),
    ("bf16 (3, 256) chain_inputs off", "bf16", (3, 256), {"chain_inputs": False}),
    ("bf16 (3, 256) fused_heads off", "bf16", (3, 256), {"fused_heads": False}),
    ("f32 (3, 256) in chunks, MAX_POINTS = 512", "f32", (3, 256), {"MAX_POINTS": 512}),
]


class Recorder(object):
    """the library, every launch entry logged with its arguments as the C side receives them"""

    def __init__(self, real):
        self.real, self.log, self.ids, self.keep = real, None, {}, []

    def begin(self):
        self.log, self.ids, self.keep = [], {}, []

    def end(self):
        log, self.log = self.log, None
        return log

    def ordinal(self, kind, handle, owner=None):
        if not handle:
            return "null"
        self.keep.append(owner)              # an object that is alive cannot share its address with a later one
        return "%s%d" % (kind, self.ids.setdefault((kind, handle), len(self.ids)))

    def arg(self, a, ctype):
        v = a.value if isinstance(a, ctypes._SimpleCData) else a
        if ctype is ctypes.c_void_p:
            return self.ordinal("p", v)       # buffers and streams: one address space
        return ctype(v).value                 # as converted: 0.125 as the float it becomes

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if name.endswith("_scratch_bytes") or name in ("dispu_linear_plan", "dispu_error_string", "dispu_version"):
            return fn

        def call(*args):
            if self.log is not None:
                assert len(args) == len(fn.argtypes), name
                self.log.append([name] + [self.arg(a, t) for a, t in zip(args, fn.argtypes)])
            return fn(*args)
        return call


def install(rec):
    """route _lib.lib() through rec and log the stream / event operations of torch.cuda"""
    import torch
    from dispu_amd import _lib
    _lib.lib = lambda: rec
    stream_of = lambda s: rec.ordinal("p", (torch.cuda.current_stream() if s is None else s).cuda_stream)
    record, wait_event, wait_stream = torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream

    def event_record(self, stream=None):
        if rec.log is not None:
            rec.log.append(["Event.record", rec.ordinal("e", id(self), self), stream_of(stream)])
        return record(self) if stream is None else record(self, stream)

    def stream_wait_event(self, event):
        if rec.log is not None:
            rec.log.append(["Stream.wait_event", stream_of(self), rec.ordinal("e", id(event), event)])
        return wait_event(self, event)

    def stream_wait_stream(self, stream):
        if rec.log is not None:
            rec.log.append(["Stream.wait_stream", stream_of(self), stream_of(stream)])
        return wait_stream(self, stream)

    torch.cuda.Event.record, torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream = event_record, stream_wait_event, stream_wait_stream


def run(out):
    import torch
    from dispu_amd import _lib, synth
    from dispu_amd.generator import Generator
    from oracle import generator as OG
    dev = torch.device("cuda:0")
    rec = Recorder(_lib.lib())
    install(rec)
    P = OG.init_params(seed=7, bias_scale=0.05, bn_random=True)
    res = {}
    for name, dtype, (B, N), attrs in CASES:
        gen = Generator(params=P, device=dev, dtype=dtype)
        for k, v in attrs.items():
            setattr(gen, k, torch.zeros(v, device=dev) if k == "fine_out" else v)
        x = torch.from_numpy(synth.patches(B, N, seed=100 + N)).to(dev)
        res[name] = {}
        for temp in ("cold", "warm"):
            rec.begin()
            gen(x)
            res[name][temp] = rec.end()
        torch.cuda.synchronize()
        print("%-45s cold %3d calls, warm %3d" % (name, len(res[name]["cold"]), len(res[name]["warm"])), flush=True)
    with open(out, "w") as f:
        json.dump(res, f)


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = sorted(set(A) ^ set(B))
    print("| case | calls cold | calls warm | equal |\n|---|---|---|---|")
    for name in A:
        if name not in B:
            continue
        same = A[name] == B[name]
        print("| %s | %d / %d | %d / %d | %s |" % (name, len(A[name]["cold"]), len(B[name]["cold"]), len(A[name]["warm"]), len(B[name]["warm"]),
                                                  "yes" if same else "NO"))
        if not same:
            bad.append(name)
            for temp in ("cold", "warm"):
                for i, (u, v) in enumerate(zip(A[name][temp], B[name][temp])):
                    if u != v:
                        print("  first difference, %s call %d:\n    %s\n    %s" % (temp, i, u, v))
                        break
    print("%d cases, %s" % (len(A), "all equal" if not bad else "DIFFERENT: %s" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    run(args.out or "generator_launches.json")
