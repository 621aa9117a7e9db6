"""Weight tables with one fault each, for the loaders that answer through pndf_table_fault (csrc/pndf_net_plan.h): pndf_load_weights on
both kernel families, pndf_skel_load_weights, pndf_cpu_load_weights and the stateless packers.  A table is what the C ABI takes:
(tensors, numel, n_tensors) in state-dict order.  A wrong size is always one element SHORT of a buffer that is whole, and the count
fault one tensor short, so that a loader which read a faulty table anyway would still stay inside the caller's memory."""
from ctypes import c_int64, c_void_p

from posendf_amd.engine import _tensor_table

# fault -> the finding of pndf_table_fault that answers it
FAULTS = ("tensors null", "numel null", "count off by one", "one tensor null", "encoder tensor of the wrong size", "trunk weight of the wrong size",
          "trunk bias of the wrong size", "dfnet-only table")
NULL_TABLE, NULL_TENSOR = ("tensors null", "numel null"), ("one tensor null",)


def good_table(sd, parents=None):
    """(keepalive, tensors, numel, n_tensors) of a state dict"""
    arrs, ptrs, numel = _tensor_table(sd, parents)
    return arrs, ptrs, numel, len(arrs)


def faulty_tables(sd, parents=None):
    """yields (fault, keepalive, tensors, numel, n_tensors) for every fault of FAULTS the network has (one with the structure encoder
    has them all)"""
    arrs, ptrs, numel, n = good_table(sd, parents)
    n_enc = sum(1 for k in sd if k.startswith("enc."))
    yield "tensors null", arrs, None, numel, n
    yield "numel null", arrs, ptrs, None, n
    yield "count off by one", arrs, ptrs, numel, n - 1

    def edited(i, null=False, short=False):
        p, m = (c_void_p * n)(*ptrs), (c_int64 * n)(*numel)
        if null:
            p[i] = None
        if short:
            m[i] -= 1
        return arrs, p, m, n

    yield ("one tensor null",) + edited(min(5, n - 1), null=True)
    if n_enc:
        yield ("encoder tensor of the wrong size",) + edited(2, short=True)
    yield ("trunk weight of the wrong size",) + edited(n_enc, short=True)
    yield ("trunk bias of the wrong size",) + edited(n_enc + 3, short=True)
    if n_enc:      # the table of the same network without its encoder (model.StrEnc.use = False)
        yield "dfnet-only table", arrs, (c_void_p * (n - n_enc))(*ptrs[n_enc:]), (c_int64 * (n - n_enc))(*numel[n_enc:]), n - n_enc
