"""numpy restatement of pam::DataManager::validate / validate_all (pam_core/DataManager.h:408-509).  TEST INFRASTRUCTURE ONLY.

    validate(name)      = validate_nan, validate_inf, validate_pos, in this order (:419-423)
    validate_single_nan   std::isnan(x)   -> "WARNING: NaN discovered in: <name> at global index: <i>"            (:471-479)
    validate_single_inf   std::isinf(x)   -> "WARNING: inf discovered in: <name> at global index: <i>"            (:484-492)
    validate_single_pos   x < 0. where the entry is positive
                          -> "WARNING: negative value discovered in positive-definite entry: <name> at global index: <i>"  (:497-509)
    die_on_failed_check   endrun("") after the first line: std::cerr << "" << std::endl, then the throw (pam_const.h:249-252)

NaN and inf are looked for in the floating kinds only (an integer converted to double is neither), negatives in every kind; bool and
whatever else is not double, float, int or long long is not looked at.  tests/golden/validate_ref.json pins `lines` to the reference.
"""
import numpy as np

KINDS = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3}
KIND_DTYPES = [np.float64, np.float32, np.int32, np.int64]
UINTS = {0: np.uint64, 1: np.uint32, 2: np.uint32, 3: np.uint64}
NAN_LINE = "WARNING: NaN discovered in: %s at global index: %d"
INF_LINE = "WARNING: inf discovered in: %s at global index: %d"
NEG_LINE = "WARNING: negative value discovered in positive-definite entry: %s at global index: %d"


def masks(array, positive):
    """boolean masks (NaN, inf, negative) of the flattened array, or None for a dtype the check skips"""
    a = np.asarray(array).reshape(-1)
    if a.dtype not in KINDS:
        return None
    none = np.zeros(a.shape, dtype=bool)
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            return np.isnan(a), np.isinf(a), (a < 0) if positive else none
    return none, none, (a < 0) if positive else none


def scan(array, positive):
    """(count[3], first[3]) as int64: the number of offenders of each class and the lowest flat index of one (-1: none)"""
    m = masks(array, positive)
    count, first = np.zeros(3, dtype=np.int64), np.full(3, -1, dtype=np.int64)
    if m is None:
        return count, first
    for c in range(3):
        idx = np.flatnonzero(m[c])
        count[c] = idx.size
        if idx.size:
            first[c] = idx[0]
    return count, first


def lines(name, array, positive, die=False):
    """what validate(name, die) writes to stderr, as a list of lines, and whether it ended in endrun (its empty line is the last entry)"""
    m = masks(array, positive)
    out = []
    if m is None:
        return out, False
    for mask, fmt in zip(m, (NAN_LINE, INF_LINE, NEG_LINE)):
        for i in np.flatnonzero(mask):
            out.append(fmt % (name, i))
            if die:
                out.append("")
                return out, True
    return out, False


def lines_all(entries, die=False):
    """validate_all(die): `entries` = [(name, array, positive)] in registration order"""
    out = []
    for name, array, positive in entries:
        got, died = lines(name, array, positive, die)
        out += got
        if died:
            return out, True
    return out, False
