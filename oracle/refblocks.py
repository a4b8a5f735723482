"""ctypes binding of oracle/_ref/libdvbt_blocks_ref.so: the REFERENCE's own blocks, compiled unmodified against the stand-in headers of
oracle/ref_standin/ and driven by oracle/ref_driver.cc (oracle/Makefile target `ref`) -- and, with which="hip", of oracle/_ref/libdvbt_shells_hip.so: the
same driver and stand-ins around the project's GNU Radio block shells (gr_dvbt_amd/host/gr), which run on libdvbt_hip.so and so need a GPU.

TEST INFRASTRUCTURE ONLY.  Either library exists only where the reference tree was at hand when `make ref` ran; available() says so.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = {"ref": os.path.join(_HERE, "_ref", "libdvbt_blocks_ref.so"), "hip": os.path.join(_HERE, "_ref", "libdvbt_shells_hip.so")}
_lib = {}
WORK_THREW = -1000                              # refblk_work's return where the shell threw (ref_driver.cc)


class ShellError(RuntimeError):
    """a shell's constructor or general_work threw; the text is the exception's what()"""


def available(which="ref"):
    return os.path.exists(_SO[which])


def lib(which="ref"):
    if which not in _lib:
        L = C.CDLL(_SO[which])
        L.refblk_make.restype = C.c_void_p
        L.refblk_make.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.c_int, C.c_float]
        L.refblk_free.argtypes = [C.c_void_p]
        L.refblk_output_multiple.argtypes = [C.c_void_p]
        L.refblk_relative_rate.argtypes = [C.c_void_p]
        L.refblk_relative_rate.restype = C.c_double
        L.refblk_itemsize.argtypes = [C.c_void_p, C.c_int]
        L.refblk_forecast.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.refblk_add_input_tag.argtypes = [C.c_void_p, C.c_int, C.c_ulonglong, C.c_char_p, C.c_long]
        L.refblk_nitems_read.argtypes = [C.c_void_p, C.c_int]
        L.refblk_nitems_read.restype = C.c_ulonglong
        L.refblk_nitems_written.argtypes = [C.c_void_p, C.c_int]
        L.refblk_nitems_written.restype = C.c_ulonglong
        L.refblk_work.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_int,
                                  C.POINTER(C.c_int)]
        L.refblk_n_output_tags.argtypes = [C.c_void_p]
        L.refblk_output_tag.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong), C.c_char_p, C.c_int, C.POINTER(C.c_long)]
        if which == "hip":
            L.refblk_last_error.restype = C.c_char_p
            L.refblk_tag_propagation_policy.argtypes = [C.c_void_p]
            L.refblk_nstreams.argtypes = [C.c_void_p, C.c_int, C.c_int]
            L.refblk_set_input_state.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        _lib[which] = L
    return _lib[which]


class Block:
    """One reference block.  args: the integer arguments of its make(), in its own order; gain: its float argument."""

    def __init__(self, name, args, gain=0.0, nin=1, nout=1, which="ref"):
        self.L = lib(which)
        self.which = which
        a = (C.c_int * len(args))(*[int(x) for x in args])
        self.h = self.L.refblk_make(name.encode(), a, len(args), C.c_float(gain))
        if not self.h:
            if which == "hip":
                raise ShellError(self.L.refblk_last_error().decode())
            raise ValueError("no reference block %r with %d arguments" % (name, len(args)))
        self.nin, self.nout = nin, nout
        if which == "hip":                                                             # a shell is driven on the streams it declares
            self.nin, self.nout = min(nin, self.L.refblk_nstreams(self.h, 0, 1)), min(nout, self.L.refblk_nstreams(self.h, 1, 1))
        self.in_itemsize = self.L.refblk_itemsize(self.h, 0)
        self.out_itemsize = self.L.refblk_itemsize(self.h, 1)
        self.output_multiple = self.L.refblk_output_multiple(self.h)
        self.relative_rate = self.L.refblk_relative_rate(self.h)

    def hints(self, noutputs):
        """what the block asks of the scheduler, as tests/golden/ref_blocks.json keeps it: forecast as [[noutput, [required per input]], ...]"""
        return {"output_multiple": self.output_multiple, "relative_rate": self.relative_rate, "in_itemsize": self.in_itemsize,
                "out_itemsize": self.out_itemsize, "forecast": [[int(n), self.forecast(int(n))] for n in sorted(set(noutputs))]}

    def tag_propagation_policy(self):
        return self.L.refblk_tag_propagation_policy(self.h)

    def set_input_state(self, done, items, port=0):
        self.L.refblk_set_input_state(self.h, port, int(done), int(items))

    def close(self):
        self.__del__()

    def __del__(self):
        if getattr(self, "h", None):
            self.L.refblk_free(self.h)
            self.h = None

    def forecast(self, noutput):
        r = (C.c_int * self.nin)()
        self.L.refblk_forecast(self.h, noutput, r, self.nin)
        return list(r)

    def tag(self, offset, key, value, port=0):
        self.L.refblk_add_input_tag(self.h, port, offset, key.encode(), value)

    def nitems_read(self, port=0):
        return self.L.refblk_nitems_read(self.h, port)

    def work(self, noutput, ins, nvisible):
        """one general_work call.  ins: one C-contiguous uint8 array per input, beginning at the item the block reads next and exposing nvisible items.
        returns (what the call returned, items consumed per input, one uint8 array of noutput items per output)"""
        outs = [np.zeros(max(noutput, 1) * self.out_itemsize + 64, np.uint8) for _ in range(self.nout)]
        ni = (C.c_int * self.nin)(*([nvisible] * self.nin))
        ip = (C.c_void_p * self.nin)(*[x.ctypes.data for x in ins[:self.nin]])
        op = (C.c_void_p * self.nout)(*[x.ctypes.data for x in outs])
        cons = (C.c_int * self.nin)()
        r = self.L.refblk_work(self.h, noutput, ni, ip, self.nin, op, self.nout, cons)
        if r == WORK_THREW and self.which == "hip":
            raise ShellError(self.L.refblk_last_error().decode())
        return r, list(cons), [o[:max(r, 0) * self.out_itemsize] for o in outs]

    def out_tags(self):
        tags = []
        port, off, val = C.c_int(), C.c_ulonglong(), C.c_long()
        key = C.create_string_buffer(64)
        for i in range(self.L.refblk_n_output_tags(self.h)):
            self.L.refblk_output_tag(self.h, i, C.byref(port), C.byref(off), key, 64, C.byref(val))
            tags.append([port.value, off.value, key.value.decode(), val.value])
        return tags

    def stream(self, ins, nitems, calls, visible=None, pad_items=4):
        """Drive the block over `nitems` input items the way a scheduler would: call after call with noutput_items taken from `calls` (the last entry
        repeats), each exposing what forecast asks for (visible=None) or `visible` items, until the input left is less than that.
        ins: one uint8 array per input.  returns {"out": [bytes per output], "log": [[noutput, returned, consumed], ...], "tags": [...], "hints": hints()
        with forecast at every noutput_items of the log}"""
        ins = [np.concatenate([np.ascontiguousarray(x, np.uint8).reshape(-1), np.zeros(pad_items * self.in_itemsize, np.uint8)]) for x in ins]
        pos, outs, log, ci = 0, [[] for _ in range(self.nout)], [], 0
        while True:
            n = calls[min(ci, len(calls) - 1)]
            need = max(self.forecast(n)) if visible is None else visible
            if pos + need > nitems:
                break
            r, cons, o = self.work(n, [x[pos * self.in_itemsize:] for x in ins], need)
            log.append([n, r, cons[0]])
            for j in range(self.nout):
                outs[j].append(o[j])
            pos += cons[0]
            ci += 1
            if r <= 0 and cons[0] == 0:
                break
        return {"out": [np.concatenate(x) if x else np.zeros(0, np.uint8) for x in outs], "log": log, "tags": self.out_tags(),
                "hints": self.hints([e[0] for e in log])}
