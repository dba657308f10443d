"""
Redundancy filtering and nearest-neighbour identities of alignment files on the GPU: the file layer over
`plm.redundancy_filter` / `plm.cross_identities`, the `run_hhfilter` drop-in for the reference's
`evcouplings.align.tools.run_hhfilter` (align/tools.py:616-680, called by modify_alignment when `seqid_filter` is set,
align/protocol.py:884-900), and a command line:

    python -m evcouplings_amd.seqfilter IN.a2m -o OUT.a3m --id 90 [--columns first|a2m] [--denominator shorter]
    python -m evcouplings_amd.seqfilter IN.a2m --against NATURAL.a2m --report OUT.csv [--id 80]

NOT VERIFIED AGAINST HHSUITE.  No `hhfilter` binary exists on any machine this project is built on, so its exact
conventions could not be compared: which denominator its sequence identity uses, what it does with a pair exactly at
the threshold (here: such a pair counts as similar and the later sequence is dropped), and the order in which it
visits the sequences (here: input order, first sequence always kept).  `denominator="shorter"` is the default of the
drop-in by recollection of HHsuite only; it is a switch ("columns", "both", "shorter") for exactly that reason.
What is verified is the definition stated in include/plm_hip.h, against a numpy twin (tests/identity_twin.py).

The arithmetic runs in libplm_hip on the GPU; reading, column selection and writing are host-side format conversion.
"""
import os

import numpy as np

from evcouplings_amd import alignment_io

GAP = ord("-")


def read_alignment(path):
    """-> (ids, chars): the headers and the N x C uint8 character matrix of a FASTA / A2M file (all rows one length)."""
    ids, seqs = alignment_io.read_fasta_records(path)
    width = len(seqs[0])
    for name, s in zip(ids, seqs):
        if len(s) != width:
            raise alignment_io.AlignmentFormatError(
                "%s: sequence %s has %d columns, the first has %d" % (path, name, len(s), width))
    chars = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), width)
    return ids, chars


def match_columns(chars, columns="a2m"):
    """Boolean mask of the match columns, decided on the first sequence as hhfilter's -M does: "first" = columns where
    it has a residue (a letter of either case), "a2m" = columns where it holds an uppercase letter or '-'."""
    first = chars[0]
    upper = (first >= ord("A")) & (first <= ord("Z"))
    lower = (first >= ord("a")) & (first <= ord("z"))
    if columns == "first":
        return upper | lower
    if columns == "a2m":
        return upper | (first == GAP)
    raise ValueError("Invalid column selection: {}".format(columns))


def match_states(chars, cols):
    """The match columns as integer states for the kernels: the ASCII code of the uppercased residue, '-' (also for
    '.') the gap state GAP; anything above 126 is refused."""
    m = np.array(chars[:, cols])
    if m.size and m.max() > 126:
        raise alignment_io.AlignmentFormatError("non-ASCII character in the alignment")
    low = (m >= ord("a")) & (m <= ord("z"))
    m[low] -= 32
    m[m == ord(".")] = GAP
    return m.astype(np.int8)


def write_a3m(path, ids, chars, cols, keep):
    """The kept sequences in A3M: match columns uppercase with '-' for gaps, the other columns as inserts (lowercase,
    their gaps dropped) -- what the reference's Alignment.from_file(f, "a3m") reads back."""
    folder = os.path.dirname(os.path.abspath(path))
    os.makedirs(folder, exist_ok=True)
    out = np.array(chars)
    up = (out >= ord("A")) & (out <= ord("Z"))
    low = (out >= ord("a")) & (out <= ord("z"))
    out[low & cols[None, :]] -= 32
    out[(out == ord(".")) & cols[None, :]] = GAP
    out[up & ~cols[None, :]] += 32
    drop = ~cols[None, :] & ((out == ord(".")) | (out == GAP))
    with open(path, "wb") as f:
        for s in np.flatnonzero(keep):
            f.write(b">" + ids[s].encode("ascii", "replace") + b"\n" + out[s][~drop[s]].tobytes() + b"\n")
    return path


def run_hhfilter(input_file, output_file, threshold=95, columns="a2m", binary=None, denominator="shorter"):
    """
    Drop-in for the reference's run_hhfilter (align/tools.py:616-680), without HHsuite: reads the FASTA / A2M
    `input_file`, takes the match columns by `columns` ("first" / "a2m", see match_columns), runs the greedy redundancy
    filter on them in input order (the first sequence is always kept; a sequence is dropped when a kept earlier one
    has identity >= threshold percent to it) and writes the kept sequences to `output_file` in A3M.  Returns
    output_file.  `binary` is accepted and ignored.  Raises ValueError for an invalid `columns`, ResourceError for a
    missing or empty input.

    NOT VERIFIED AGAINST HHSUITE: no hhfilter binary exists on any machine this project is built on.  The
    denominator of its identity ("shorter" here, by recollection only; `denominator` switches it), its treatment of a
    pair exactly at the threshold, and its internal ordering are therefore assumptions -- see the module docstring.
    """
    from evcouplings_amd import plm
    from evcouplings_amd.tools import ResourceError
    if columns not in ("first", "a2m"):
        raise ValueError("Invalid column selection: {}".format(columns))
    if not (os.path.isfile(input_file) and os.path.getsize(input_file) > 0):
        raise ResourceError("Alignment file does not exist or is empty: {}".format(input_file))
    ids, chars = read_alignment(input_file)
    cols = match_columns(chars, columns)
    if not cols.any():
        raise ResourceError("no match columns in {} (columns={})".format(input_file, columns))
    keep = plm.redundancy_filter(match_states(chars, cols), float(threshold) / 100.0, gap_state=GAP,
                                 denominator=denominator)
    return write_a3m(output_file, ids, chars, cols, keep)


def nearest_report(input_file, against_file, report_file, threshold=80, columns="a2m", denominator="columns"):
    """CSV (id, nearest_id, identity, n_within) of every sequence of input_file against the sequences of
    against_file; both files must have the same number of match columns."""
    from evcouplings_amd import plm
    ids_a, chars_a = read_alignment(input_file)
    ids_b, chars_b = read_alignment(against_file)
    a = match_states(chars_a, match_columns(chars_a, columns))
    b = match_states(chars_b, match_columns(chars_b, columns))
    if a.shape[1] != b.shape[1]:
        raise alignment_io.AlignmentFormatError(
            "%s has %d match columns, %s has %d" % (input_file, a.shape[1], against_file, b.shape[1]))
    r = plm.cross_identities(a, b, threshold=float(threshold) / 100.0, gap_state=GAP, denominator=denominator)
    with open(report_file, "w") as f:
        f.write("id,nearest_id,identity,n_within\n")
        for k, name in enumerate(ids_a):
            near = ids_b[r["best_index"][k]] if r["best_index"][k] >= 0 else ""
            f.write("%s,%s,%.6f,%d\n" % (name.split()[0], near.split()[0] if near else "", r["identity"][k],
                                         r["n_within"][k]))
    return report_file


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog="python -m evcouplings_amd.seqfilter", description=__doc__.split("\n\n")[0])
    p.add_argument("input", help="FASTA / A2M alignment")
    p.add_argument("-o", "--output", help="filtered alignment (A3M)")
    p.add_argument("--id", type=float, default=None, help="identity threshold in percent (filter: 95, report: 80)")
    p.add_argument("--columns", choices=("first", "a2m"), default="a2m")
    p.add_argument("--denominator", choices=("columns", "both", "shorter"), default=None)
    p.add_argument("--against", help="second alignment: report the nearest of its sequences for every input sequence")
    p.add_argument("--report", help="CSV written with --against")
    args = p.parse_args(argv)
    if bool(args.against) != bool(args.report):
        p.error("--against and --report go together")
    if not args.against and not args.output:
        p.error("give -o OUT.a3m (filter) or --against / --report (nearest identities)")
    if args.output:
        run_hhfilter(args.input, args.output, threshold=95 if args.id is None else args.id, columns=args.columns,
                     denominator=args.denominator or "shorter")
    if args.against:
        nearest_report(args.input, args.against, args.report, threshold=80 if args.id is None else args.id,
                       columns=args.columns, denominator=args.denominator or "columns")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
