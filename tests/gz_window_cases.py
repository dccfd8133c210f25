"""Models shared by tests/test_gz_window_host.py, tests/test_gpu_gz_window.py and tests/test_cli_gz_windows.py: gz windows. Data and models
only; built with the helpers of gz_cases.py and gz_files_cases.py.

    walk_windows(b, ...)     the model of csrc/gz_plan.h gz_next_window, called until it yields no window
    plan_window(...)         the model of gz_plan_window
    cut_windows(b, ...)      [window bytes] of a well-formed file, by the walker's rule with a bound on the text alone
    chain(...)               the model of a chain of windows: what every window's batch, carry, bytes and lines must be"""
import struct

import gz_cases as G
import gz_files_cases as F

LIMIT = 1 << 31


def walk_windows(b, max_comp, max_text, max_member):
    """([(end, members, text, [cuts])], stop): the windows gz_next_window yields over the file b from 0 on, and where it yields none"""
    cuts = F.split_members(b)
    ends = cuts[1:] + [len(b)]
    out, k, frm = [], 0, 0
    while frm < len(b):
        # the header at `frm`: any string length for the file's first, SPLIT_MAX_STR behind it (a cut's header has parsed that way already)
        if F.parse_header(b, frm, max_str=None if frm == 0 else F.SPLIT_MAX_STR) is None:
            break
        text, mine = 0, []
        while k < len(cuts):
            at, end = cuts[k], ends[k]
            body = F.parse_header(b, at, max_str=None if at == 0 else F.SPLIT_MAX_STR)
            mlen = end - at
            if mlen - (body - at) < 8 or mlen > max_member:
                break
            isize = struct.unpack("<I", b[end - 4:end])[0]
            if isize > max_member or text + isize > max_text or end - frm > max_comp:
                break
            mine.append(at)
            text += isize
            k += 1
        if not mine:
            break
        out.append((ends[k - 1], len(mine), text, mine))
        frm = ends[k - 1]
    return out, frm


def plan_window(blob, carry_len, last):
    """the model of gz_plan_window: (members [(status, cap, start)], caps, total), or None where the plan refuses the batch"""
    members, first, starts, caps, _ = F.plan_files([blob])
    run = 0
    for _, status, cap, start in members:                    # gz_plan_files itself refuses: the same rule without the carry
        run += cap
        if run + 1 >= LIMIT:
            return None
    if carry_len + caps[0] + 1 >= LIMIT:
        return None
    text = carry_len + caps[0]
    return [(status, cap, start + carry_len) for _, status, cap, start in members], caps[0], text + (1 if last and text else 0)


def cut_windows(b, max_text):
    """the windows of a well-formed file as byte strings: whole members, at most max_text bytes of text each (one member at least)"""
    windows, stop = walk_windows(b, 1 << 40, max_text, 1 << 40)
    assert stop == len(b), "a member alone is above max_text"
    out, at = [], 0
    for end, _, _, _ in windows:
        out.append(b[at:end])
        at = end
    return out


def chain(texts, carry_cap):
    """texts: the inflated text of every window of a file, in order (the last one is the file's LAST window). The model of the chain:
    [(carry_in, batch, carry_out, bytes, lines, status)] — batch is what gz_text() must be, with the tail blanked and the separator of
    the last window. Stops behind the first window with NO_LINE_END (status 1)."""
    out, carry = [], b""
    for k, t in enumerate(texts):
        last = k + 1 == len(texts)
        whole = carry + t
        if last:
            batch = whole + (b"\n" if whole else b"")
            out.append((carry, batch, b"", len(whole), whole.count(b"\n"), 0))
            break
        nl = whole.rfind(b"\n")
        tail = whole[nl + 1:]
        if len(tail) > carry_cap:                            # also nl == -1 in a window longer than the cap
            out.append((carry, b"\n" * len(whole), b"", 0, 0, 1))
            break
        keep = whole[:len(whole) - len(tail)]
        out.append((carry, keep + b"\n" * len(tail), tail, len(keep), keep.count(b"\n"), 0))
        carry = tail
    return out
