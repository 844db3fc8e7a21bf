"""ctypes binding of libmirprefer.so (include/mirprefer.h).

There is no CPU fallback: if the shared library is missing or no GPU is usable, the calls raise."""
import ctypes as C
import os

import numpy as np

from . import early
from .early import LIB_PATH, FastaData, SamData, TailedSamData
ABI_VERSION = 17     # include/mirprefer.h as this binding was written against (mirp_abi_version of the library must match)


class MirpError(RuntimeError):
    pass


class FoldLine(C.Structure):
    _fields_ = [("start", C.c_int32), ("len", C.c_int32), ("energy", C.c_int32), ("printed", C.c_int32)]


class Region(C.Structure):
    _fields_ = [("tid", C.c_int32), ("start", C.c_int32), ("end", C.c_int32)]


class TrimOpts(C.Structure):
    """MirpTrimOpts of include/mirprefer.h."""
    _fields_ = [("adapter", C.c_char * 64)] + [(f, C.c_int32) for f in ("adapter_len", "error_permille", "min_overlap", "quality_cutoff", "min_length",
                                                                       "max_length", "discard_untrimmed", "reserved")]


TRIM_STATS = ("reads", "quality_trimmed", "adapter", "untrimmed", "too_short", "too_long", "written")


class LibqcOpts(C.Structure):
    """MirpLibqcOpts of include/mirprefer.h."""
    _fields_ = [("adapter", C.c_char * 64)] + [(f, C.c_int32) for f in ("adapter_len", "error_permille", "min_overlap", "reserved")] + [("sample", C.c_int64)]


class LibqcFound(C.Structure):
    """MirpLibqcFound of include/mirprefer.h."""
    _fields_ = ([("adapter", C.c_char * 64)] + [(f, C.c_int32) for f in ("adapter_len", "status", "seed_code", "left_steps", "left_stop", "reserved")] +
                [("seed_count", C.c_int64), ("min_count", C.c_int64)])


LIBQC_STATS = ("reads", "sampled", "with_adapter", "dimers")
LIBQC_STATUS = ("none", "ok", "unsure")               # MIRP_LIBQC_NONE, _OK, _UNSURE
LIBQC_STOPS = ("purity", "support", "cap")
LIBQC_SAMPLE = 1 << 20


class TargetOpts(C.Structure):
    """MirpTargetOpts of include/mirprefer.h."""
    _fields_ = [("max_half_score", C.c_int32), ("both_strands", C.c_int32), ("cleavage_site", C.c_int32), ("bulge", C.c_int32), ("max_sites", C.c_int64),
                ("energy", C.c_int32), ("accessibility", C.c_int32)]


TARGET_STATS = ("mirnas", "targets", "bases", "evaluations", "sites", "passes")


class MimicOpts(C.Structure):
    """MirpMimicOpts of include/mirprefer.h."""
    _fields_ = [("max_imperfect", C.c_int32), ("loop_len", C.c_int32), ("both_strands", C.c_int32), ("reserved", C.c_int32), ("max_sites", C.c_int64)]


MIMIC_STATS = ("mirnas", "no_seed", "targets", "bases", "seeds", "entries", "sites", "passes")


class AnnotateOpts(C.Structure):
    """MirpAnnotateOpts of include/mirprefer.h."""
    _fields_ = [("max_offset", C.c_int32), ("max_mismatches", C.c_int32), ("n_species", C.c_int32), ("reserved", C.c_int32), ("max_lines", C.c_int64),
                ("species", C.c_char_p)]


ANNOTATE_STATS = ("queries", "known", "skipped", "pairs", "evaluations", "hits", "identical", "isomir", "homolog", "novel", "lines", "passes")


class RandfoldOpts(C.Structure):
    """MirpRandfoldOpts of include/mirprefer.h."""
    _fields_ = [("seed", C.c_uint64), ("n_shuffles", C.c_int32), ("dinucleotide", C.c_int32), ("capacity", C.c_int64)]


# MirpRandfoldRec of include/mirprefer.h: one sequence of mirp_randfold
RANDFOLD_DTYPE = np.dtype([("len", "<i4"), ("gc", "<i4"), ("mfe", "<i4"), ("le", "<i4"), ("min_mfe", "<i4"), ("reserved", "<i4"), ("sum", "<i8"),
                           ("sum_sq", "<i8")])
RANDFOLD_STATS = ("sequences", "folds", "passes", "fallbacks")

# MirpDuplexRec of include/mirprefer.h: one pair of mirp_duplex_batch
DUPLEX_DTYPE = np.dtype([("mfe", "<i4"), ("pairs", "<i4"), ("a_first", "<i4"), ("a_last", "<i4"), ("b_first", "<i4"), ("b_last", "<i4")])
DUPLEX_STATS = ("pairs", "passes", "evaluations")


class EnsembleOpts(C.Structure):
    """MirpEnsembleOpts of include/mirprefer.h."""
    _fields_ = [("bpp_cutoff", C.c_double), ("want_bpp", C.c_int32), ("reserved", C.c_int32)]


# MirpEnsembleRec of include/mirprefer.h: one sequence of mirp_ensemble
ENSEMBLE_DTYPE = np.dtype([("len", "<i4"), ("mfe", "<i4"), ("efe", "<f8"), ("mfe_freq", "<f8"), ("diversity", "<f8"), ("centroid_dist", "<f8"),
                           ("centroid_pairs", "<i4"), ("reserved", "<i4")])
# MirpBpp of include/mirprefer.h: one pair of mirp_ensemble's list, positions 1-based
BPP_DTYPE = np.dtype([("seq", "<i4"), ("i", "<i4"), ("j", "<i4"), ("reserved", "<i4"), ("p", "<f8")])
ENSEMBLE_STATS = ("sequences", "passes", "cells")

class HairpinOpts(C.Structure):
    """MirpHairpinOpts of include/mirprefer.h."""
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open", C.c_int32), ("gap_extend", C.c_int32), ("min_score", C.c_int32),
                ("reserved", C.c_int32), ("max_lines", C.c_int64)]


# MirpHairpinHit of include/mirprefer.h: one hit of mirp_hairpin_align, positions 1-based and inclusive
HAIRPIN_DTYPE = np.dtype([(f, "<i4") for f in ("query", "known", "score", "q_start", "q_end", "k_start", "k_end", "matches", "mismatches", "gap_opens",
                                               "gap_bases", "reserved")])
HAIRPIN_STATS = ("queries", "known", "pairs", "cells", "hits", "passes", "score_passes", "trace_passes")
HAIRPIN_STRIP = 16          # MIRP_HAIRPIN_STRIP of include/mirprefer.h: query rows a lane of the scoring kernel holds in registers

class InvertedOpts(C.Structure):
    """MirpInvertedOpts of include/mirprefer.h."""
    _fields_ = [("max_span", C.c_int32), ("min_score", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32), ("gap", C.c_int32), ("reserved", C.c_int32)]


# MirpInvertedRec of include/mirprefer.h: one inverted repeat, positions 1-based and inclusive within its contig
INVERTED_DTYPE = np.dtype([("contig", "<i4"), ("score", "<i4"), ("left_start", "<i8"), ("left_end", "<i8"), ("right_start", "<i8"), ("right_end", "<i8"),
                           ("matches", "<i4"), ("mismatches", "<i4"), ("gaps", "<i4"), ("reserved", "<i4")])
INVERTED_STATS = ("contigs", "bases", "cells", "rows_above", "candidates", "traced", "dropped_untraced", "accepted", "scan_passes", "trace_passes", "tiles")
INVERTED_TILE = 8192          # MIRP_INVERTED_TILE of include/mirprefer.h: rows a wave of the row scan owns
INVERTED_STRIP = 1024         # MIRP_INVERTED_STRIP: rows the 64 lanes of a wave hold at once
INVERTED_MAX_SPAN = 4096      # MIRP_INVERTED_MAX_SPAN: the largest max_span


class NatsOpts(C.Structure):
    """MirpNatsOpts of include/mirprefer.h."""
    _fields_ = [(f, C.c_int32) for f in ("seed", "band", "max_occ", "min_seeds", "match", "mismatch", "gap", "min_score", "min_length", "reserved")]


# MirpNatsRec of include/mirprefer.h: one complementary region of the transcripts a < b, positions 1-based and inclusive in each transcript's own sense
NATS_DTYPE = np.dtype([(f, "<i4") for f in ("a", "b", "score", "a_start", "a_end", "a_len", "b_start", "b_end", "b_len", "matches", "mismatches", "gaps",
                                            "seeds", "bin")])
NATS_STATS = ("transcripts", "skipped", "bases", "kmers_ignored", "seed_hits", "candidates", "kept_candidates", "cells", "above", "traced", "regions",
              "pairs", "join_passes", "scan_launches", "trace_passes")
NATS_MAX_LEN = 65535          # MIRP_NATS_MAX_LEN of include/mirprefer.h: the longest transcript that is searched
NATS_FAMILY = 8               # the band scan's family of mirp_last_jobs_per_slot

class AlignPlaceOpts(C.Structure):
    """MirpAlignPlaceOpts of include/mirprefer.h."""
    _fields_ = [("mode", C.c_int32), ("window", C.c_int32), ("seed", C.c_uint64)]


class AlignTailOpts(C.Structure):
    """MirpAlignTailOpts of include/mirprefer.h."""
    _fields_ = [("max_tail", C.c_int32), ("min_templated", C.c_int32), ("trim", C.c_int32), ("reserved", C.c_int32)]


class HomologOpts(C.Structure):
    """MirpHomologOpts of include/mirprefer.h."""
    _fields_ = [("max_mismatches", C.c_int32), ("precursor_len", C.c_int32), ("max_placements", C.c_int32), ("reserved", C.c_int32)]


# MirpHomologRec of include/mirprefer.h: one locus of mirp_homolog_scan, coordinates 1-based with exclusive ends
HOMOLOG_DTYPE = np.dtype([(f, "<i4") for f in ("query", "contig", "strand", "mismatches", "mat_s", "mat_e", "star_s", "star_e", "fold_s", "fold_e", "win_s",
                                               "win_e", "prime5", "total_bps", "total_dots", "energy", "line_len", "ss_len", "n_also", "reserved")] +
                         [("text_off", "<i8"), ("also_off", "<i8")])
HOMOLOG_STATS = ("queries", "repeat_like", "placements", "passing", "loci", "scan_passes", "chunks", "folds", "eval_reruns", "eval_global_text")

# MirpUnpairedRec of include/mirprefer.h: one window of mirp_unpaired_batch, kcal/mol
UNPAIRED_DTYPE = np.dtype([("efe", "<f8"), ("efe_open", "<f8"), ("upe", "<f8")])
SORT_REC_DTYPE = np.dtype([("key", "<u8"), ("a", "<u4"), ("b", "<u4")])      # MirpSortRec (mirp_sort_records)
UNPAIRED_STATS = ("windows", "passes", "cells")


class PhaseOpts(C.Structure):
    """MirpPhaseOpts of include/mirprefer.h."""
    _fields_ = [(f, C.c_int32) for f in ("length", "cycles", "min_phased", "min_depth")]


# MirpPhaseWindow of include/mirprefer.h: one passing window of mirp_phase_scan
PHASE_WINDOW_DTYPE = np.dtype([("tid", "<i4"), ("n", "<i4"), ("k", "<i4"), ("reserved", "<i4"), ("start", "<i8"), ("phased_reads", "<i8"),
                               ("window_reads", "<i8")])


class TriggerOpts(C.Structure):
    """MirpTriggerOpts of include/mirprefer.h."""
    _fields_ = [(f, C.c_int32) for f in ("length", "cycles", "min_phased", "min_depth", "max_half_score", "drift")]


# MirpTriggerLocus and MirpTrigger of include/mirprefer.h: one locus interval and one trigger of mirp_trigger_scan
TRIGGER_LOCUS_DTYPE = np.dtype([("tid", "<i4"), ("contig", "<i4"), ("start", "<i8"), ("end", "<i8")])
TRIGGER_DTYPE = np.dtype([("locus", "<i4"), ("mirna", "<i4"), ("half", "<i4"), ("strand", "<i4"), ("side", "<i4"), ("offset", "<i4"), ("n", "<i4"),
                          ("k", "<i4"), ("pos", "<i8"), ("phased_reads", "<i8"), ("window_reads", "<i8")])
TRIGGER_STATS = ("mirnas", "interval_bases", "sites", "windows", "records", "units")


class ClusterOpts(C.Structure):
    """MirpClusterOpts of include/mirprefer.h."""
    _fields_ = [("threshold", C.c_int64), ("pad", C.c_int64), ("contig_len", C.c_void_p), ("n_contigs", C.c_int32), ("n_samples", C.c_int32)]


# MirpCluster of include/mirprefer.h: one cluster of mirp_cluster_scan; sizes = depth of len < 20, 20, 21, 22, 23, 24, > 24
CLUSTER_DTYPE = np.dtype([("tid", "<i4"), ("major_strand", "<i4"), ("major_len", "<i4"), ("reserved", "<i4"), ("start", "<i8"), ("end", "<i8"),
                          ("reads", "<i8"), ("plus_reads", "<i8"), ("placements", "<i8"), ("major_pos", "<i8"), ("major_reads", "<i8"),
                          ("sizes", "<i8", (7,))])
CLUSTER_STATS = ("records", "total", "islands", "clusters", "assigned")


class LocusOpts(C.Structure):
    """MirpLocusOpts of include/mirprefer.h."""
    _fields_ = [("contig_len", C.c_void_p), ("n_contigs", C.c_int32), ("n_samples", C.c_int32), ("stranded", C.c_int32), ("reserved", C.c_int32)]


# MirpLocusSpan of include/mirprefer.h: one locus of mirp_locus_scan; strand 0 '+', 1 '-', 2 none
LOCUS_DTYPE = np.dtype([("tid", "<i4"), ("strand", "<i4"), ("start", "<i8"), ("end", "<i8")])
LOCUS_STATS = ("records", "loci", "jobs", "pairs", "max_len")
LOCI_CHUNK = 4096           # MIRP_LOCI_CHUNK of include/mirprefer.h: table rows (records, placements) one wave-job of the locus scan serves
LOCI_MAX = 1 << 24          # MIRP_LOCI_MAX


class SignatureOpts(C.Structure):
    """MirpSignatureOpts of include/mirprefer.h."""
    _fields_ = [("contig_len", C.c_void_p), ("n_contigs", C.c_int32), ("min_len", C.c_int32), ("max_len", C.c_int32), ("max_overlap", C.c_int32),
                ("overhang", C.c_int32), ("reserved", C.c_int32), ("min_reads", C.c_int64)]


# MirpSignatureRow and MirpDuplexSite of include/mirprefer.h: one row per locus and one listed duplex of mirp_signature_scan
SIGNATURE_ROW_DTYPE = np.dtype([("reads", "<i8"), ("plus_reads", "<i8"), ("duplexes", "<i8"), ("duplex_reads", "<i8"), ("major_pos", "<i8"),
                                ("major_plus", "<i8"), ("major_minus", "<i8"), ("major_len", "<i4"), ("reserved", "<i4")])
DUPLEX_SITE_DTYPE = np.dtype([("locus", "<i8"), ("pos", "<i8"), ("plus_reads", "<i8"), ("minus_reads", "<i8"), ("len", "<i4"), ("reserved", "<i4")])
SIGNATURE_STATS = ("records", "kept", "u_entries", "v_entries", "jobs", "sites")
SIGNATURE_CHUNK = 4096      # MIRP_SIGNATURE_CHUNK: table rows (U entries, placements) one wave-job of the signature scan serves
SIGNATURE_MAX_OVERLAP = 64  # MIRP_SIGNATURE_MAX_OVERLAP


class DiffexpOpts(C.Structure):
    """MirpDiffexpOpts of include/mirprefer.h."""
    _fields_ = [("size_factor", C.c_void_p), ("group", C.c_void_p), ("n_samples", C.c_int32), ("mode", C.c_int32), ("phi", C.c_double),
                ("min_mean", C.c_double), ("pseudo", C.c_double)]


# MirpDiffexpRow of include/mirprefer.h: one feature of mirp_diffexp; p = -1 marks an untested feature
DIFFEXP_DTYPE = np.dtype([(f, "<f8") for f in ("base_mean", "mean_a", "mean_b", "log2fc", "dispersion", "p")] + [("k_a", "<u8"), ("k_b", "<u8")])
DIFFEXP_STATS = ("features", "tested", "jobs", "terms", "phi_c")
DIFFEXP_MODES = ("max", "common", "feature", "fixed")      # MirpDiffexpOpts.mode 0 .. 3
DIFFEXP_CHUNK = 4096                   # MIRP_DIFFEXP_CHUNK: terms one wave-job of the test serves
DIFFEXP_MAX_FEATURES = 1 << 24         # MIRP_DIFFEXP_MAX_FEATURES
DIFFEXP_MAX_COUNT = 1 << 40            # MIRP_DIFFEXP_MAX_COUNT


class IsomirOpts(C.Structure):
    """MirpIsomirOpts of include/mirprefer.h."""
    _fields_ = [("max5", C.c_int32), ("max3", C.c_int32), ("n_samples", C.c_int32), ("reserved", C.c_int32)]


# MirpIsoLocus, MirpIsomir and MirpIsoLocusSum of include/mirprefer.h: an annotated miRNA, one isomiR and the sums of one locus of mirp_isomir_scan
ISO_LOCUS_DTYPE = np.dtype([("tid", "<i4"), ("strand", "<i4"), ("start", "<i8"), ("end", "<i8")])
ISOMIR_DTYPE = np.dtype([("locus", "<i4"), ("d5", "<i4"), ("d3", "<i4"), ("tail", "<u4"), ("reads", "<i8")])
ISO_SUM_DTYPE = np.dtype([(f, "<i8") for f in ("reads", "canonical", "shift5", "trim3", "ext3", "tailed", "tail_u", "tail_a", "isomirs", "major_reads",
                                               "major")])
ISOMIR_STATS = ("records", "assigned", "depth", "isomirs")


class DegradomeOpts(C.Structure):
    """MirpDegradomeOpts of include/mirprefer.h."""
    _fields_ = [("max_half_score", C.c_int32), ("cleavage_site", C.c_int32), ("max_category", C.c_int32), ("n_contigs", C.c_int32), ("alpha", C.c_double),
                ("contig_names", C.c_char_p), ("contig_len", C.c_void_p)]


DEGRADOME_STATS = ("mirnas", "transcripts", "bases", "records", "sense", "minus", "units", "c0", "c1", "c2", "c3", "c4", "evaluations", "hits", "passes")


def report_readmapping(loci, ss_list, alns, contig_arrays, sample_names, counts0):
    """Bodies of the per-locus read-mapping files (mirp_report_readmapping, host only): loci = int32 [n, 8] {tid, fold_s, fold_e, mat_s, mat_e,
    star_s, star_e, strand}, ss_list = n structure strings, contig_arrays[t] = uint8 bases of contig t (None / empty where not held),
    counts0 = int64 [n, n_samples] reads on the precursor.  -> list of n strings (the lines after the header line)."""
    lib = load_library()
    loci = np.ascontiguousarray(loci, dtype=np.int32).reshape(-1, 8)
    n = len(loci)
    if n == 0:
        return []
    alns = np.ascontiguousarray(alns)
    keep = [np.ascontiguousarray(a, dtype=np.uint8) if a is not None and len(a) else None for a in contig_arrays]
    ptrs = (C.c_void_p * len(keep))(*[a.ctypes.data if a is not None else None for a in keep])
    lens = np.array([len(a) if a is not None else 0 for a in keep], dtype=np.int64)
    ssb = b"".join(x.encode() + b"\0" for x in ss_list)
    snb = b"".join(x.encode() + b"\0" for x in sample_names)
    cnt = np.ascontiguousarray(counts0, dtype=np.int64)
    text, offs = C.c_void_p(), C.c_void_p()
    rc = lib.mirp_report_readmapping(loci.ctypes.data, n, ssb, alns.ctypes.data if len(alns) else None, len(alns), ptrs, lens.ctypes.data, len(keep), snb,
                                     len(sample_names), cnt.ctypes.data, C.byref(text), C.byref(offs))
    if rc != 0:
        raise MirpError("mirp_report_readmapping failed (%d): a locus lies on a contig this process does not hold" % rc)
    o = _copy_out(lib, offs, np.int64, n + 1)
    blob = C.string_at(text.value, int(o[-1]))
    lib.mirp_free(text)
    return [blob[o[k]:o[k + 1]].decode() for k in range(n)]


def write_reports(loci, contig_names, ss_list, pre_list, sample_names, counts, mirbase_form, paths):
    """The report files of the predict stage (mirp_write_reports, host only, native threads): loci = int32 [n, 10] {contig index, fold_s, fold_e, mat_s,
    mat_e, star_s, star_e, strand, star expressed, overhang code} in final order, ss_list / pre_list = n structure / forward-strand precursor strings,
    counts = int64 [n, n_samples, 4], mirbase_form = the four fixed pieces of the two miRBase search forms, paths = {"gff", "mature", "precursor",
    "ss", "csv", "html", "stat"} -> file name (missing = not written)."""
    lib = load_library()
    loci = np.ascontiguousarray(loci, dtype=np.int32).reshape(-1, 10)
    n = len(loci)
    cnt = np.ascontiguousarray(counts, dtype=np.int64).reshape(n, len(sample_names), 4)
    blob = lambda xs: b"".join(x.encode() + b"\0" for x in xs)
    p = lambda k: paths[k].encode() if paths.get(k) else None
    err = C.create_string_buffer(512)
    fn = lib.mirp_write_reports
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, C.c_void_p, C.c_char_p, C.c_int32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_char_p] + [C.c_char_p] * 7 + \
                  [C.c_char_p, C.c_size_t]
    rc = fn(n, loci.ctypes.data if n else None, blob(contig_names), len(contig_names), blob(ss_list), blob(pre_list), blob(sample_names), len(sample_names),
            cnt.ctypes.data if cnt.size else None, blob(mirbase_form), p("gff"), p("mature"), p("precursor"), p("ss"), p("csv"), p("html"), p("stat"), err, 512)
    if rc != 0:
        raise MirpError("%s (%d)" % (err.value.decode(), rc))


def write_result_reports(result, text, contig_names, contig_arrays, alns, sample_names, mirbase_form, outdir, prefix):
    """The tail of the predict stage in one native call (mirp_write_result_reports, host only): result = MIRNA_DTYPE records and text = their structure
    rows as Context.predict_raw returns them, contig_arrays[t] = uint8 bases of contig t (None / empty where not held).  Writes readmapping/ and the
    seven report files under outdir.  -> (records in list order after the mature/star swap, order[n] = input index of list position i,
    counts int64 [n, n_samples, 4])."""
    lib = load_library()
    result = np.ascontiguousarray(result)
    n = len(result)
    text = np.ascontiguousarray(text, dtype=np.uint8).reshape(n, -1) if n else np.zeros((0, 1), np.uint8)
    alns = np.ascontiguousarray(alns)
    keep = [np.ascontiguousarray(a, dtype=np.uint8) if a is not None and len(a) else None for a in contig_arrays]
    ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data if a is not None else None for a in keep])
    lens = np.array([len(a) if a is not None else 0 for a in keep] or [0], dtype=np.int64)
    blob = lambda xs: b"".join(x.encode() + b"\0" for x in xs)
    order = np.zeros(max(n, 1), dtype=np.int32)
    out = np.zeros(max(n, 1), dtype=result.dtype)
    counts = np.zeros((max(n, 1), len(sample_names), 4), dtype=np.int64)
    err = C.create_string_buffer(512)
    fn = lib.mirp_write_result_reports
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int32, C.c_char_p,
                   C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
    rc = fn(result.ctypes.data if n else None, n, text.ctypes.data if n else None, int(text.shape[1]), blob(contig_names), len(contig_names), ptrs, lens.ctypes.data,
            alns.ctypes.data if len(alns) else None, len(alns), blob(sample_names), len(sample_names), blob(mirbase_form), str(outdir).encode(), str(prefix).encode(),
            order.ctypes.data, out.ctypes.data, counts.ctypes.data, err, 512)
    if rc != 0:
        raise MirpError("%s (%d)" % (err.value.decode(), rc))
    return out[:n], order[:n], counts[:n]


def write_files(paths, texts, n_threads=1):
    """mirp_write_files: file paths[k] <- texts[k] (str), written natively, outside the interpreter lock."""
    lib = load_library()
    n = len(paths)
    if n == 0:
        return
    enc = [t.encode() for t in texts]
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=offs[1:])
    err = C.create_string_buffer(512)
    fn = lib.mirp_write_files
    fn.restype = C.c_int
    fn.argtypes = [C.c_int64, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_size_t]
    rc = fn(n, b"".join(p.encode() + b"\0" for p in paths), b"".join(enc), offs.ctypes.data, int(n_threads), err, 512)
    if rc != 0:
        raise MirpError("%s (%d)" % (err.value.decode(), rc))


def read_fasta(path, want=None):
    """Native FASTA reader (mirp_read_fasta): -> list of (name, uint8 array) in file order; with `want` (names) only those sequences are
    materialised, the others come back as None."""
    lib = load_library()
    got = early.take_fasta(path) if not want else None      # the CLI may have started this read before the heavy imports (early.py)
    if got is not None:
        rc, d, msg = got
        if rc != 0:
            raise ValueError(msg)
    else:
        d = FastaData()
        err = C.create_string_buffer(512)
        nw = len(want) if want else 0
        arr = (C.c_char_p * max(nw, 1))(*[str(w).encode() for w in (want or [])])
        if lib.mirp_read_fasta(str(path).encode(), arr, nw, C.byref(d), err, 512) != 0:
            raise ValueError(err.value.decode())
    keep = got is not None          # the CLI's early read: the process is short-lived, the arrays below are views of the library's buffer (no 119 MB copy
    try:                            # at config[2]); the buffer is never handed back -- _FASTA_KEEP holds the descriptor until the process ends
        raw = np.frombuffer((C.c_char * d.n_bytes).from_address(d.seq), dtype=np.uint8, count=d.n_bytes) if d.n_bytes else np.zeros(0, np.uint8)
        blob = raw if keep else raw.copy()
        out, off, o = [], 0, 0
        for k in range(d.n_contigs):
            nm = C.string_at(d.names + off)
            off += len(nm) + 1
            L = d.len[k]
            if L < 0:
                out.append((nm.decode(), None))
            else:
                out.append((nm.decode(), blob[o:o + L])); o += L
    finally:
        if keep:
            _FASTA_KEEP.append(d)
        else:
            lib.mirp_free_fasta_data(C.byref(d))
    return out


_FASTA_KEEP = []


class _SamHold:
    """Owns the buffers of one MirpSamData until the record arrays that view them are gone (mirp_free_sam_data then)."""

    def __init__(self, lib, d):
        self.lib, self.d = lib, d

    def __del__(self):
        try:
            self.lib.mirp_free_sam_data(C.byref(self.d))
        except Exception:
            pass


def _unpack_sam_data(lib, d):
    """-> (contig names, lengths, sample names, alns, segs).  The record arrays are VIEWS of the library's buffers (no copy of 16 bytes x 10^7 records:
    the copy was half of the ingest leg's wall-clock); the buffers are released when the last array viewing them is collected."""
    from .synth import ALN_DTYPE
    hold = _SamHold(lib, d)

    def names(ptr, n):
        out, off = [], 0
        for _ in range(n):
            s = C.string_at(ptr + off)
            out.append(s.decode()); off += len(s) + 1
        return out
    cn = names(d.contig_names, d.n_contigs)
    sn = names(d.sample_names, d.n_samples)
    lens = np.array([d.contig_len[k] for k in range(d.n_contigs)], dtype=np.int64)

    def recs(ptr, n):
        if not n:
            return np.zeros(0, dtype=ALN_DTYPE)
        buf = (C.c_char * (n * 16)).from_address(ptr)
        buf._hold = hold          # the array's base keeps the owner alive
        return np.frombuffer(buf, dtype=ALN_DTYPE, count=n)
    alns, segs = recs(d.alns, d.n_alns), recs(d.segs, d.n_segs)
    return cn, lens, sn, alns, segs


def tokenize_sams_tailed(paths, n_threads=0):
    """The tailed SAM tokenizer of the isomiR counts (mirp_tokenize_sams_tailed; threads, no device): every kept record as its templated
    footprint (pos = POS, len = m of `<m>M`) and the code of its 3' tail, in (sample, file) order.  Adopts the run the CLI started before its heavy
    imports (early.start_tailed).  -> (contig names, lengths, sample names, alns, uint32 tail codes, {cigar, long_tail} skipped records)."""
    from .synth import ALN_DTYPE
    lib = load_library()
    got = early.take_tailed(paths)
    if got is not None:
        rc, d, msg = got
    else:
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        d = TailedSamData()
        err = C.create_string_buffer(512)
        rc = lib.mirp_tokenize_sams_tailed(arr, len(paths), int(n_threads), C.byref(d), err, 512)
        msg = err.value.decode()
    if rc != 0:
        raise ValueError(msg)
    try:
        def names(ptr, n):
            out, off = [], 0
            for _ in range(n):
                b = C.string_at(ptr + off)
                out.append(b.decode()); off += len(b) + 1
            return out
        cn, sn = names(d.contig_names, d.n_contigs), names(d.sample_names, d.n_samples)
        lens = np.array([d.contig_len[k] for k in range(d.n_contigs)], dtype=np.int64)
        n = d.n_alns
        alns = np.frombuffer((C.c_char * (n * 16)).from_address(d.alns), dtype=ALN_DTYPE, count=n).copy() if n else np.zeros(0, dtype=ALN_DTYPE)
        tails = np.frombuffer((C.c_char * (n * 4)).from_address(d.tails), dtype="<u4", count=n).copy() if n else np.zeros(0, dtype="<u4")
        skipped = {"cigar": int(d.skipped_cigar), "long_tail": int(d.skipped_long_tail)}
    finally:
        lib.mirp_free_tailed_sam_data(C.byref(d))
    return cn, lens, sn, alns, tails, skipped


def ingest_sams(paths, n_threads=0, with_segments=False):
    """Native multi-threaded SAM ingest, host sort (mirp_ingest_sams). -> (contig_names, contig_lens, sample_names, alns[, segs])."""
    lib = load_library()
    arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
    d = SamData()
    err = C.create_string_buffer(512)
    if lib.mirp_ingest_sams(arr, len(paths), int(n_threads), C.byref(d), err, 512) != 0:
        raise ValueError(err.value.decode())
    out = _unpack_sam_data(lib, d)
    return out if with_segments else out[:4]


FOLD_LINE_DTYPE = np.dtype([("start", "<i4"), ("len", "<i4"), ("energy", "<i4"), ("printed", "<i4")])


def fold_window_lines(raw, w):
    """(lines, ss) record arrays of window w of a Context.get_fold() result: the side buffer for a window that needed more
    lines than the main buffers hold, its slot in the main buffers otherwise."""
    ov = raw.get("overflow")
    if ov and int(w) in ov:
        return ov[int(w)]
    return raw["lines"][w], raw["ss"][w]

_lib = None


def load_library():
    """Load libmirprefer.so; raises MirpError loudly when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MirpError("libmirprefer.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(there is no CPU fallback for the product path)")
    lib = early.cdll()
    lib.mirp_abi_version.argtypes = []
    lib.mirp_abi_version.restype = C.c_int
    if lib.mirp_abi_version() != ABI_VERSION:      # a stale build (or a stale MIRP_LIB variant) would be called through the wrong signatures
        raise MirpError("%s has ABI version %d, this binding needs %d: rebuild it (make -C mir-prefer_amd/csrc)" % (LIB_PATH, lib.mirp_abi_version(), ABI_VERSION))
    if os.environ.get("MIRP_LIB"):
        import sys
        sys.stderr.write("[mirp] using the library named by MIRP_LIB: %s\n" % LIB_PATH)
    vp = C.c_void_p
    lib.mirp_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.mirp_create.restype = C.c_int
    lib.mirp_destroy.argtypes = [vp]
    lib.mirp_destroy.restype = None
    lib.mirp_last_error.argtypes = [vp]
    lib.mirp_last_error.restype = C.c_char_p
    lib.mirp_free.argtypes = [vp]
    lib.mirp_free.restype = None
    lib.mirp_abi_version.argtypes = []
    lib.mirp_abi_version.restype = C.c_int
    lib.mirp_fold_batch.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int32), C.POINTER(vp),
                                    C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_fold_batch.restype = C.c_int
    lib.mirp_fold_batch_summary.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_fold_batch_summary.restype = C.c_int
    lib.mirp_predict_batch.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int32, C.c_int32, vp, vp,
                                       C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_predict_batch.restype = C.c_int
    lib.mirp_predict_batch_reasons.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_int32, C.c_int32, vp, vp,
                                               C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    lib.mirp_predict_batch_reasons.restype = C.c_int
    i64p, i32p = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    lib.mirp_load_genome.argtypes = [vp, C.c_int32, vp, vp]
    lib.mirp_load_alignments.argtypes = [vp, vp, C.c_int64]
    lib.mirp_candidate.argtypes = [vp, vp, vp, i64p, i64p, i64p]
    lib.mirp_get_depth.argtypes = [vp, C.POINTER(vp), i64p]
    lib.mirp_get_peaks.argtypes = [vp, C.POINTER(vp), i64p]
    lib.mirp_get_loci.argtypes = [vp, C.POINTER(vp), i64p, C.POINTER(vp), i64p]
    lib.mirp_get_windows.argtypes = [vp, C.POINTER(vp), i64p, C.POINTER(vp), i64p, C.POINTER(vp), i64p, C.POINTER(vp), i64p]
    lib.mirp_fold.argtypes = [vp, C.c_int32, C.c_int32]
    lib.mirp_set_fold_model.argtypes = [vp, C.c_int32]
    lib.mirp_set_contig_shard.argtypes = [vp, C.c_int32]
    lib.mirp_set_contig_shard.restype = C.c_int
    lib.mirp_set_fold_model.restype = C.c_int
    lib.mirp_get_fold.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i32p, i32p, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_predict.argtypes = [vp, vp, C.POINTER(vp), i64p, C.POINTER(vp), i32p, C.POINTER(vp), C.POINTER(vp), i64p]
    lib.mirp_get_fold_overflow.argtypes = [vp, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp), i32p, i32p, C.POINTER(vp)]
    lib.mirp_get_fold_overflow.restype = C.c_int
    lib.mirp_predict_reasons.argtypes = [vp, vp, C.POINTER(vp), i64p, i32p]
    lib.mirp_predict_reasons.restype = C.c_int
    lib.mirp_last_timings.argtypes = [vp, C.POINTER(C.c_double)]
    lib.mirp_last_fold_fallbacks.argtypes = [vp]
    lib.mirp_last_fold_fallbacks.restype = C.c_int64
    lib.mirp_get_window_readtable.argtypes = [vp, C.POINTER(vp), i32p, i64p]
    lib.mirp_get_window_readtable.restype = C.c_int
    lib.mirp_last_fold_kernel_ms.argtypes = [vp, C.POINTER(C.c_double)]
    lib.mirp_last_fold_kernel_ms.restype = C.c_int
    lib.mirp_microbench.argtypes = [vp, C.POINTER(C.c_double)]
    lib.mirp_microbench.restype = C.c_int
    lib.mirp_last_fold_overflow.argtypes = [vp]
    lib.mirp_last_fold_overflow.restype = C.c_int64
    lib.mirp_last_coverage_fused.argtypes = [vp]
    lib.mirp_last_coverage_fused.restype = C.c_int
    lib.mirp_set_coverage_path.argtypes = [vp, C.c_int32]
    lib.mirp_set_coverage_path.restype = C.c_int
    lib.mirp_limit_windows.argtypes = [vp, C.c_int64]
    lib.mirp_limit_windows.restype = C.c_int
    lib.mirp_exchange_bytes.argtypes = [vp, vp, vp, C.POINTER(vp), vp]
    lib.mirp_exchange_bytes.restype = C.c_int
    lib.mirp_set_fold_split_path.argtypes = [vp, C.c_int32]
    lib.mirp_set_fold_split_path.restype = C.c_int
    lib.mirp_set_fold_overlap.argtypes = [vp, C.c_int32]
    lib.mirp_set_fold_overlap.restype = C.c_int
    lib.mirp_set_fold_overlap_tailfree.argtypes = [vp, C.c_int32]
    lib.mirp_set_fold_overlap_tailfree.restype = C.c_int
    lib.mirp_set_fold_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_fold_capacity.restype = C.c_int
    lib.mirp_last_fold_overlap_chunks.argtypes = [vp]
    lib.mirp_last_fold_overlap_chunks.restype = C.c_int
    lib.mirp_last_fold_dense.argtypes = [vp]
    lib.mirp_last_fold_dense.restype = C.c_int64
    lib.mirp_set_fold_dedup.argtypes = [vp, C.c_int32]
    lib.mirp_set_fold_dedup.restype = C.c_int
    lib.mirp_set_fold_dedup_hash_bits.argtypes = [vp, C.c_int32]
    lib.mirp_set_fold_dedup_hash_bits.restype = C.c_int
    lib.mirp_last_fold_duplicates.argtypes = [vp]
    lib.mirp_last_fold_duplicates.restype = C.c_int64
    lib.mirp_get_fold_duplicates.argtypes = [vp, C.POINTER(vp), i64p]
    lib.mirp_get_fold_duplicates.restype = C.c_int
    lib.mirp_write_fold_text.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.mirp_write_fold_text.restype = C.c_int
    lib.mirp_write_fold_text_async.argtypes = [vp, C.c_char_p, C.c_char_p]
    lib.mirp_write_fold_text_async.restype = C.c_int
    lib.mirp_wait_text.argtypes = [vp]
    lib.mirp_wait_text.restype = C.c_int
    for f in ("mirp_write_depth_text", "mirp_write_window_fasta"):
        getattr(lib, f).argtypes = [vp, C.c_char_p, C.c_char_p, C.c_int32]
        getattr(lib, f).restype = C.c_int
    lib.mirp_get_fold_summary.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64p]
    lib.mirp_get_fold_summary.restype = C.c_int
    for f in ("mirp_load_genome", "mirp_load_alignments", "mirp_candidate", "mirp_get_depth", "mirp_get_peaks", "mirp_get_loci",
              "mirp_get_windows", "mirp_fold", "mirp_get_fold", "mirp_predict", "mirp_last_timings"):
        getattr(lib, f).restype = C.c_int
    lib.mirp_ingest_sams.argtypes = [C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.POINTER(SamData), C.c_char_p, C.c_size_t]
    lib.mirp_ingest_sams.restype = C.c_int
    lib.mirp_free_sam_data.argtypes = [C.POINTER(SamData)]
    lib.mirp_free_sam_data.restype = None
    lib.mirp_ingest_sams_gpu.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, vp, C.c_int64, C.POINTER(SamData), C.POINTER(C.c_double)]
    lib.mirp_ingest_sams_gpu.restype = C.c_int
    lib.mirp_load_coverage_segments.argtypes = [vp, vp, C.c_int64]
    lib.mirp_load_coverage_segments.restype = C.c_int
    lib.mirp_ingest_sams_shard.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, vp, C.c_int64, vp, C.POINTER(SamData), C.POINTER(C.c_double)]
    lib.mirp_ingest_sams_shard.restype = C.c_int
    lib.mirp_report_readmapping.argtypes = [vp, C.c_int64, C.c_char_p, vp, C.c_int64, vp, vp, C.c_int32, C.c_char_p, C.c_int32, vp, C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_report_readmapping.restype = C.c_int
    lib.mirp_read_fasta.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(FastaData), C.c_char_p, C.c_size_t]
    lib.mirp_read_fasta.restype = C.c_int
    lib.mirp_free_fasta_data.argtypes = [C.POINTER(FastaData)]
    lib.mirp_free_fasta_data.restype = None
    lib.mirp_collapse_reads.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, i64p, i64p, C.POINTER(C.c_double)]
    lib.mirp_collapse_reads.restype = C.c_int
    lib.mirp_last_collapse_collisions.argtypes = [vp]
    lib.mirp_last_collapse_collisions.restype = C.c_int64
    lib.mirp_align_index.argtypes = [vp, C.POINTER(C.c_char_p), C.c_int32, i32p, i64p, C.POINTER(C.c_double)]
    lib.mirp_align_index.restype = C.c_int
    lib.mirp_align_reads.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, i64p, C.POINTER(C.c_double)]
    lib.mirp_align_reads.restype = C.c_int
    lib.mirp_align_last_batches.argtypes = [vp]
    lib.mirp_align_last_batches.restype = C.c_int64
    lib.mirp_align_reads_placed.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(AlignPlaceOpts),
                                            i64p, C.POINTER(C.c_double)]
    lib.mirp_align_reads_placed.restype = C.c_int
    lib.mirp_align_reads_tailed.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.POINTER(AlignTailOpts), i64p, C.POINTER(C.c_double)]
    lib.mirp_align_reads_tailed.restype = C.c_int
    lib.mirp_set_align_place_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_align_place_capacity.restype = C.c_int
    lib.mirp_align_place_last_realigned.argtypes = [vp]
    lib.mirp_align_place_last_realigned.restype = C.c_int64
    lib.mirp_trim_reads.argtypes = [vp, C.c_char_p, C.c_int64, C.c_char_p, C.POINTER(TrimOpts), C.c_char_p, i64p, C.POINTER(C.c_double)]
    lib.mirp_trim_reads.restype = C.c_int
    lib.mirp_trim_last_paths.argtypes = [vp, i64p]
    lib.mirp_trim_last_paths.restype = C.c_int
    lib.mirp_libqc_reads.argtypes = [vp, C.c_char_p, C.c_int64, C.c_char_p, C.POINTER(LibqcOpts), C.POINTER(LibqcFound), i64p, i64p, i64p, i64p,
                                     C.POINTER(C.c_double)]
    lib.mirp_libqc_reads.restype = C.c_int
    lib.mirp_libqc_last_table.argtypes = [vp, C.c_void_p]
    lib.mirp_libqc_last_table.restype = C.c_int
    lib.mirp_target_scan.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(TargetOpts), C.c_char_p, i64p, C.POINTER(C.c_double)]
    lib.mirp_target_scan.restype = C.c_int
    lib.mirp_mimic_scan.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(MimicOpts), C.c_char_p, i64p, C.POINTER(C.c_double)]
    lib.mirp_mimic_scan.restype = C.c_int
    lib.mirp_annotate_scan.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.POINTER(AnnotateOpts), C.c_char_p, C.c_char_p, i64p,
                                       C.POINTER(C.c_double)]
    lib.mirp_annotate_scan.restype = C.c_int
    lib.mirp_randfold.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(RandfoldOpts), C.POINTER(vp), i64p, C.POINTER(C.c_double)]
    lib.mirp_randfold.restype = C.c_int
    lib.mirp_shuffle_batch.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(RandfoldOpts), C.c_int32, C.c_int32, C.POINTER(vp), i64p]
    lib.mirp_shuffle_batch.restype = C.c_int
    lib.mirp_duplex_batch.argtypes = [vp, C.c_char_p, i64p, C.c_char_p, i64p, C.c_int32, vp, vp]
    lib.mirp_duplex_batch.restype = C.c_int
    lib.mirp_set_duplex_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_duplex_capacity.restype = C.c_int
    lib.mirp_duplex_last_stats.argtypes = [vp, i64p]
    lib.mirp_duplex_last_stats.restype = C.c_int
    lib.mirp_ensemble.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(EnsembleOpts), vp, vp, C.POINTER(vp), i64p]
    lib.mirp_ensemble.restype = C.c_int
    lib.mirp_set_ensemble_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_ensemble_capacity.restype = C.c_int
    lib.mirp_ensemble_last_stats.argtypes = [vp, i64p]
    lib.mirp_ensemble_last_stats.restype = C.c_int
    lib.mirp_unpaired_batch.argtypes = [vp, C.c_char_p, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, vp]
    lib.mirp_unpaired_batch.restype = C.c_int
    lib.mirp_set_unpaired_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_unpaired_capacity.restype = C.c_int
    lib.mirp_unpaired_last_stats.argtypes = [vp, i64p]
    lib.mirp_unpaired_last_stats.restype = C.c_int
    lib.mirp_unpaired_lds_longest.argtypes = []
    lib.mirp_unpaired_lds_longest.restype = C.c_int
    lib.mirp_hairpin_align.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.c_char_p, i64p, C.c_int32, C.POINTER(HairpinOpts), C.POINTER(vp), i64p, C.POINTER(vp),
                                       C.POINTER(vp)]
    lib.mirp_hairpin_align.restype = C.c_int
    lib.mirp_set_hairpin_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_hairpin_capacity.restype = C.c_int
    lib.mirp_hairpin_last_stats.argtypes = [vp, i64p, C.POINTER(C.c_double), i64p]
    lib.mirp_hairpin_last_stats.restype = C.c_int
    lib.mirp_inverted_scan.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(InvertedOpts), C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_inverted_scan.restype = C.c_int
    lib.mirp_set_inverted_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_inverted_capacity.restype = C.c_int
    lib.mirp_inverted_last_stats.argtypes = [vp, i64p, C.POINTER(C.c_double)]
    lib.mirp_inverted_last_stats.restype = C.c_int
    lib.mirp_nats_scan.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(NatsOpts), C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_nats_scan.restype = C.c_int
    lib.mirp_set_nats_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_nats_capacity.restype = C.c_int
    lib.mirp_nats_last_stats.argtypes = [vp, i64p, C.POINTER(C.c_double)]
    lib.mirp_nats_last_stats.restype = C.c_int
    lib.mirp_homolog_scan.argtypes = [vp, C.c_char_p, i64p, C.c_int32, C.POINTER(HomologOpts), C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp)]
    lib.mirp_homolog_scan.restype = C.c_int
    lib.mirp_homolog_contigs.argtypes = [vp, C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(C.c_int32)]
    lib.mirp_homolog_contigs.restype = C.c_int
    lib.mirp_set_homolog_capacity.argtypes = [vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.mirp_set_homolog_capacity.restype = C.c_int
    lib.mirp_homolog_last_stats.argtypes = [vp, i64p, C.POINTER(C.c_double)]
    lib.mirp_homolog_last_stats.restype = C.c_int
    lib.mirp_last_jobs_per_slot.argtypes = [vp, C.c_int32, i64p]
    lib.mirp_last_jobs_per_slot.restype = C.c_int
    lib.mirp_set_target_flanks.argtypes = [vp, C.c_int32, C.c_int32]
    lib.mirp_set_target_flanks.restype = C.c_int
    lib.mirp_set_target_capacity.argtypes = [vp, C.c_int64]
    lib.mirp_set_target_capacity.restype = C.c_int
    lib.mirp_phase_scan.argtypes = [vp, C.POINTER(PhaseOpts), vp, C.POINTER(vp), i64p, i64p]
    lib.mirp_phase_scan.restype = C.c_int
    lib.mirp_trigger_scan.argtypes = [vp, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, vp, C.c_int64, C.POINTER(TriggerOpts), vp, C.POINTER(vp), i64p,
                                      vp, i64p, C.POINTER(C.c_double)]
    lib.mirp_trigger_scan.restype = C.c_int
    lib.mirp_cluster_scan.argtypes = [vp, C.POINTER(ClusterOpts), C.POINTER(vp), i64p, C.POINTER(vp), i64p]
    lib.mirp_cluster_scan.restype = C.c_int
    lib.mirp_locus_scan.argtypes = [vp, vp, C.c_int64, C.POINTER(LocusOpts), C.POINTER(vp), C.POINTER(vp), i64p]
    lib.mirp_locus_scan.restype = C.c_int
    lib.mirp_signature_scan.argtypes = [vp, vp, C.c_int64, C.POINTER(SignatureOpts), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), i64p, i64p]
    lib.mirp_signature_scan.restype = C.c_int
    lib.mirp_diffexp.argtypes = [vp, vp, C.c_int64, C.POINTER(DiffexpOpts), C.POINTER(vp), i64p]
    lib.mirp_diffexp.restype = C.c_int
    lib.mirp_tokenize_sams_tailed.argtypes = [C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.POINTER(TailedSamData), C.c_char_p, C.c_size_t]
    lib.mirp_tokenize_sams_tailed.restype = C.c_int
    lib.mirp_free_tailed_sam_data.argtypes = [C.POINTER(TailedSamData)]
    lib.mirp_free_tailed_sam_data.restype = None
    lib.mirp_isomir_scan.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(IsomirOpts), C.POINTER(vp), i64p, C.POINTER(vp), C.POINTER(vp),
                                     C.POINTER(vp), i64p]
    lib.mirp_isomir_scan.restype = C.c_int
    lib.mirp_degradome_scan.argtypes = [vp, C.c_char_p, C.c_char_p, C.POINTER(DegradomeOpts), C.c_char_p, i64p, C.POINTER(C.c_double)]
    lib.mirp_degradome_scan.restype = C.c_int
    lib.mirp_dist_unique_id.argtypes = [vp]
    lib.mirp_dist_unique_id.restype = C.c_int
    lib.mirp_dist_init.argtypes = [vp, vp, C.c_int32, C.c_int32]
    lib.mirp_dist_init.restype = C.c_int
    lib.mirp_dist_init_local.argtypes = [vp, C.c_char_p, C.c_int32, C.c_int32]
    lib.mirp_dist_init_local.restype = C.c_int
    for f in ("mirp_dist_finalize", "mirp_dist_barrier", "mirp_dist_rank", "mirp_dist_world"):
        getattr(lib, f).argtypes = [vp]
        getattr(lib, f).restype = C.c_int
    lib.mirp_dist_comm_info.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.mirp_dist_comm_info.restype = C.c_int
    lib.mirp_dist_allreduce_sum.argtypes = [vp, vp, C.c_int32]
    lib.mirp_dist_allreduce_sum.restype = C.c_int
    lib.mirp_gather_loci.argtypes = [vp, C.c_int32, C.POINTER(vp), i64p, C.POINTER(vp), i32p]
    lib.mirp_gather_loci.restype = C.c_int
    lib.mirp_gather_records.argtypes = [vp, vp, C.c_int64, C.c_int32, C.c_int32, C.POINTER(vp), i64p]
    lib.mirp_gather_records.restype = C.c_int
    _lib = lib
    return lib


def cigar_of(ops):
    """ops (bytes, one of = X I D per alignment column) -> their run-length encoding, e.g. b"===II=" -> "3=2I1=" """
    out, i = [], 0
    while i < len(ops):
        j = i
        while j < len(ops) and ops[j] == ops[i]:
            j += 1
        out.append("%d%s" % (j - i, chr(ops[i])))
        i = j
    return "".join(out)


def _copy_out(lib, ptr, dtype, count):
    if count == 0:
        arr = np.zeros(0, dtype=dtype)
    else:
        nbytes = int(count) * np.dtype(dtype).itemsize
        buf = (C.c_char * nbytes).from_address(ptr.value)
        arr = np.frombuffer(buf, dtype=dtype, count=count).copy()
    lib.mirp_free(ptr)
    return arr


class Context:
    """One device context (maps onto the reference's process-per-piece model)."""

    def __init__(self, device=0):
        self.lib = load_library()
        got = early.take_context(int(device))      # the CLI may have started the context before the heavy imports (early.py)
        if got is not None:
            rc, h = got
        else:
            h = C.c_void_p()
            rc = self.lib.mirp_create(int(device), C.byref(h))
        if rc != 0:
            raise MirpError("mirp_create(device=%d) failed with code %d (no usable GPU?)" % (device, rc))
        self.h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.mirp_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise MirpError("%s failed (%d): %s" % (what, rc, self.lib.mirp_last_error(self.h).decode()))

    def collapse_reads(self, path, prefix, out_path, hash_bits=64):
        """process-reads-fasta.py on one file (mirp_collapse_reads): writes out_path, returns {n_reads, n_unique, collisions, seconds}; seconds =
        {read + upload, split, hash + sort, verify + rank, emit + download, write}.  hash_bits < 64 only to force hash collisions in tests."""
        nr, nu = C.c_int64(), C.c_int64()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_collapse_reads(self.h, os.fsencode(path), prefix.encode(), os.fsencode(out_path), int(hash_bits), C.byref(nr), C.byref(nu), sec),
                    "mirp_collapse_reads")
        return {"n_reads": nr.value, "n_unique": nu.value, "collisions": int(self.lib.mirp_last_collapse_collisions(self.h)), "seconds": list(sec)}

    def align_index(self, paths):
        """bowtie-build on the reference FASTA files, in order (mirp_align_index): the index stays on the device for later align_reads calls.
        -> {n_contigs, total, seconds}; seconds = {read + parse + pack, upload, keys, sort, positions + buckets}."""
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        nc, tot = C.c_int32(), C.c_int64()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_align_index(self.h, arr, len(paths), C.byref(nc), C.byref(tot), sec), "mirp_align_index")
        return {"n_contigs": nc.value, "total": tot.value, "seconds": list(sec)}

    def align_reads(self, reads_path, out_path, pg_cl="", v=0, k=20, m=0, filter_unmapped=False, place=0, window=50, seed=0, tail=0, tail_min=16,
                    tail_trim=False, tails_path=None):
        """bowtie -v v --best --strata -k k [-m m] -S on one read FASTA file against the index of align_index (mirp_align_reads): writes out_path.
        m = 0: no -m.  -> {reads, aligned, unaligned, suppressed, records, seconds}; seconds = {read + parse, upload, seeds, verify, sort,
        emit + download + write}.  A large file runs in several batches on the device; align_last_batches() tells how many the last call took.
        place = "u" / "r" (or 1 / 2): one record per read, multi-mapped reads placed by the density of the file's unique reads within `window`
        bases, or at random (mirp_align_reads_placed; DESIGN.md §12 "Placement"); m must then be 1..10000 and k is not consulted.  The result has
        unique, by_density and at_random as well, and seconds two more entries {placement, first pass}.
        tail = 1..8: the reads left without a hit are searched for a templated 5' part of at least tail_min bases followed by at most `tail`
        non-templated bases (mirp_align_reads_tailed; DESIGN.md §12 "Tails"); tail_trim: their records hold the templated part only; the
        summary goes to tails_path (default out_path + ".tails.tsv").  The result has tailed and tail_suppressed as well, `aligned` includes
        the tailed reads, and seconds one more entry, the tail pass.  tail = 0: exactly the call without it.  Not together with place."""
        mode = {0: 0, None: 0, "u": 1, "r": 2, 1: 1, 2: 2}[place]
        if tail:
            if mode:
                raise ValueError("align_reads: tail and place cannot be combined")
            st = (C.c_int64 * 7)()
            sec = (C.c_double * 7)()
            o = AlignTailOpts(int(tail), int(tail_min), int(bool(tail_trim)), 0)
            tp = os.fsencode(out_path) + b".tails.tsv" if tails_path is None else os.fsencode(tails_path)
            self._check(self.lib.mirp_align_reads_tailed(self.h, os.fsencode(reads_path), os.fsencode(out_path), tp, pg_cl.encode(), int(v), int(k), int(m),
                                                         int(bool(filter_unmapped)), C.byref(o), st, sec), "mirp_align_reads_tailed")
            return dict(zip(("reads", "aligned", "unaligned", "suppressed", "records", "tailed", "tail_suppressed"), list(st)), seconds=list(sec))
        if mode:
            st = (C.c_int64 * 8)()
            sec = (C.c_double * 8)()
            o = AlignPlaceOpts(mode, int(window), int(seed))
            self._check(self.lib.mirp_align_reads_placed(self.h, os.fsencode(reads_path), os.fsencode(out_path), pg_cl.encode(), int(v), int(k), int(m),
                                                         int(bool(filter_unmapped)), C.byref(o), st, sec), "mirp_align_reads_placed")
            return dict(zip(("reads", "aligned", "unaligned", "suppressed", "records", "unique", "by_density", "at_random"), list(st)), seconds=list(sec))
        st = (C.c_int64 * 5)()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_align_reads(self.h, os.fsencode(reads_path), os.fsencode(out_path), pg_cl.encode(), int(v), int(k), int(m),
                                              int(bool(filter_unmapped)), st, sec), "mirp_align_reads")
        return dict(zip(("reads", "aligned", "unaligned", "suppressed", "records"), list(st)), seconds=list(sec))

    def align_last_batches(self):
        """Batches the last align_reads ran on the device (mirp_align_last_batches)."""
        return int(self.lib.mirp_align_last_batches(self.h))

    def set_align_place_capacity(self, items):
        """Hits the first pass of a placed align_reads keeps resident for the second (mirp_set_align_place_capacity); 0 = the default."""
        self._check(self.lib.mirp_set_align_place_capacity(self.h, int(items)), "mirp_set_align_place_capacity")

    def align_place_last_realigned(self):
        """Batches the last placed align_reads aligned twice (mirp_align_place_last_realigned)."""
        return int(self.lib.mirp_align_place_last_realigned(self.h))

    def trim_reads(self, data, name, out_path, adapter="", error_permille=100, overlap=3, quality=0, min_length=18, max_length=0, discard_untrimmed=False):
        """3' adapter and quality trimming of one FASTQ / FASTA text (bytes, already decompressed) (mirp_trim_reads): writes out_path,
        the FASTA of the kept reads; name is what messages call the file.  -> {reads, quality_trimmed, adapter, untrimmed, too_short, too_long,
        written, seconds}; seconds = {upload, split, records, trim, emit + download, write}."""
        o = TrimOpts()
        ad = adapter.encode() if isinstance(adapter, str) else bytes(adapter)
        o.adapter = ad
        o.adapter_len, o.error_permille, o.min_overlap, o.quality_cutoff = len(ad), int(error_permille), int(overlap), int(quality)
        o.min_length, o.max_length, o.discard_untrimmed = int(min_length), int(max_length), int(bool(discard_untrimmed))
        st = (C.c_int64 * 7)()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_trim_reads(self.h, data, len(data), os.fsencode(name), C.byref(o), os.fsencode(out_path), st, sec), "mirp_trim_reads")
        return dict(zip(TRIM_STATS, list(st)), seconds=list(sec))

    def trim_last_paths(self):
        """(workgroups that staged their reads in LDS, workgroups that read them from device memory) of the last trim_reads (mirp_trim_last_paths);
        (0, 0) after a refused call."""
        out = (C.c_int64 * 2)()
        self._check(self.lib.mirp_trim_last_paths(self.h, out), "mirp_trim_last_paths")
        return int(out[0]), int(out[1])

    def target_scan(self, mirna_path, target_paths, out_path, max_half_score=8, both_strands=False, cleavage_site=False, max_sites=0, bulge=False,
                    energy=False, accessibility=False, flanks=None):
        """Plant miRNA target sites (mirp_target_scan): every miRNA of mirna_path against the target FASTA files, in order; writes
        the TSV to out_path.  max_half_score = 2 x the -s score.  bulge: also the sites with one unpaired nucleotide, and a last column `bulge`
        on every line.  energy: the duplex free energy columns `mfe mfe_perfect mfe_ratio duplex` last on every line.  accessibility: a last
        column `upe`, the energy that opens the site's window of the target; flanks: (up, down) bases of that window beside the
        site, None = (17, 13).  -> {mirnas, targets, bases, evaluations, sites, passes, seconds}; seconds =
        {parse, upload, scan, sort + cut, emit + download + write}."""
        o = TargetOpts()
        o.max_half_score, o.both_strands, o.cleavage_site, o.max_sites = int(max_half_score), int(bool(both_strands)), int(bool(cleavage_site)), int(max_sites)
        o.bulge = int(bool(bulge))
        o.energy = int(bool(energy))
        o.accessibility = int(bool(accessibility))
        arr = (C.c_char_p * len(target_paths))(*[os.fsencode(p) for p in target_paths])
        st = (C.c_int64 * 6)()
        sec = (C.c_double * 5)()
        up, down = (17, 13) if flanks is None else flanks
        self._check(self.lib.mirp_set_target_flanks(self.h, int(up), int(down)), "mirp_set_target_flanks")
        try:
            self._check(self.lib.mirp_target_scan(self.h, os.fsencode(mirna_path), arr, len(target_paths), C.byref(o), os.fsencode(out_path), st, sec),
                        "mirp_target_scan")
        finally:
            self.lib.mirp_set_target_flanks(self.h, 17, 13)
        return dict(zip(TARGET_STATS, list(st)), seconds=list(sec))

    def set_target_capacity(self, keys):
        """Sites one target_scan pass holds on the device (0 = the default, 2^26; at least 2): lowered only to test the overflow path."""
        self._check(self.lib.mirp_set_target_capacity(self.h, int(keys)), "mirp_set_target_capacity")

    def mimic_scan(self, mirna_path, target_paths, out_path, max_imperfect=3, loop_len=3, both_strands=False, max_sites=0):
        """Endogenous target mimics (mirp_mimic_scan): every miRNA of mirna_path against the target FASTA files, in order, anchored on
        the seed (positions 2..8); writes the TSV to out_path.  max_imperfect: most mismatches + G:U pairs (0..6); loop_len: unpaired target
        bases (2..6).  -> {mirnas, no_seed, targets, bases, seeds, entries, sites, passes, seconds}; no_seed = miRNAs with an unknown letter in
        2..8 (in no bucket), seeds = 7-mers looked up, entries = bucket entries evaluated; seconds = {parse + table, upload, scan, sort + cut,
        emit + download + write}.  Passes hold at most set_target_capacity keys."""
        o = MimicOpts()
        o.max_imperfect, o.loop_len, o.both_strands, o.max_sites = int(max_imperfect), int(loop_len), int(bool(both_strands)), int(max_sites)
        arr = (C.c_char_p * len(target_paths))(*[os.fsencode(p) for p in target_paths])
        st = (C.c_int64 * 8)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_mimic_scan(self.h, os.fsencode(mirna_path), arr, len(target_paths), C.byref(o), os.fsencode(out_path), st, sec),
                    "mirp_mimic_scan")
        return dict(zip(MIMIC_STATS, list(st)), seconds=list(sec))

    def annotate_scan(self, query_path, known_paths, out_path, summary_path, max_offset=2, max_mismatches=2, max_lines=0, species=()):
        """Known-miRNA annotation (mirp_annotate_scan): every sequence of query_path against the known FASTA files, in order; writes
        the hits TSV to out_path and one line per query to summary_path.  species: prefixes of the known ids to keep (empty = all).  -> {queries,
        known, skipped, pairs, evaluations, hits, identical, isomir, homolog, novel, lines, passes, seconds}; seconds = {parse, upload, counting
        scan, key scans, sort + cut, download + write}.  Passes hold at most set_target_capacity keys."""
        o = AnnotateOpts()
        o.max_offset, o.max_mismatches, o.max_lines = int(max_offset), int(max_mismatches), int(max_lines)
        sp = [x.encode() if isinstance(x, str) else bytes(x) for x in species]
        blob = C.create_string_buffer(b"".join(x + b"\0" for x in sp) + b"\0")
        o.n_species = len(sp)
        o.species = C.cast(blob, C.c_char_p)
        arr = (C.c_char_p * len(known_paths))(*[os.fsencode(p) for p in known_paths])
        st = (C.c_int64 * 12)()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_annotate_scan(self.h, os.fsencode(query_path), arr, len(known_paths), C.byref(o), os.fsencode(out_path),
                                                os.fsencode(summary_path), st, sec), "mirp_annotate_scan")
        return dict(zip(ANNOTATE_STATS, list(st)), seconds=list(sec))

    @staticmethod
    def _randfold_input(seqs, n_shuffles, dinucleotide, seed, capacity):
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs])
        o = RandfoldOpts()
        o.seed, o.n_shuffles, o.dinucleotide, o.capacity = int(seed), int(n_shuffles), int(bool(dinucleotide)), int(capacity)
        return bs, b"".join(bs), offs, o

    def randfold(self, seqs, n_shuffles=999, dinucleotide=True, seed=0, capacity=0):
        """Shuffle test of precursor MFEs (mirp_randfold): seqs (list of str / bytes) are shuffled n_shuffles times each on the
        device, folded with this context's fold model and reduced to one record per sequence.  capacity: sequences folded per pass (0 = the
        default), lowered only in tests.  -> (RANDFOLD_DTYPE array, {sequences, folds, passes, fallbacks, seconds}); seconds = {upload, shuffle,
        fold, statistics, download}."""
        bs, blob, offs, o = self._randfold_input(seqs, n_shuffles, dinucleotide, seed, capacity)
        ptr = C.c_void_p()
        st = (C.c_int64 * 4)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_randfold(self.h, blob, offs.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o), C.byref(ptr), st, sec), "mirp_randfold")
        return _copy_out(self.lib, ptr, RANDFOLD_DTYPE, len(bs)), dict(zip(RANDFOLD_STATS, list(st)), seconds=list(sec))

    def shuffle_batch(self, seqs, k0, n_k, dinucleotide=True, seed=0, capacity=0):
        """The shuffles k0 .. k0 + n_k - 1 of every sequence as the device makes them for randfold (mirp_shuffle_batch; for tests).
        -> list (per sequence) of n_k bytes objects of ACGUN letters."""
        bs, blob, offs, o = self._randfold_input(seqs, 1, dinucleotide, seed, capacity)
        ptr, nb = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_shuffle_batch(self.h, blob, offs.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o), int(k0), int(n_k), C.byref(ptr),
                                                C.byref(nb)), "mirp_shuffle_batch")
        raw = _copy_out(self.lib, ptr, np.uint8, nb.value).tobytes()
        out, at = [], 0
        for b in bs:
            out.append([raw[at + k * len(b):at + (k + 1) * len(b)] for k in range(int(n_k))])
            at += int(n_k) * len(b)
        return out

    def duplex_batch(self, a_list, b_list, structures=True, capacity=0):
        """Two-strand minimum free energy fold (mirp_duplex_batch) of a_list[q] with b_list[q] (str / bytes, both 5'->3', 1..64 nt,
        A C G U/T in either case, anything else N), Turner-2004 whatever the context's fold model.  capacity: pairs per pass (0 = the default),
        lowered only in tests.  -> (DUPLEX_DTYPE array, [bytes] of the structure texts, or None without structures)."""
        if len(a_list) != len(b_list):
            raise ValueError("duplex_batch: %d strands a and %d strands b" % (len(a_list), len(b_list)))
        blobs, offs = [], []
        for strands in (a_list, b_list):
            bs = [s.encode() if isinstance(s, str) else bytes(s) for s in strands]
            o = np.zeros(len(bs) + 1, dtype=np.int64)
            if bs:
                o[1:] = np.cumsum([len(b) for b in bs])
            blobs.append(b"".join(bs))
            offs.append(o)
        n = len(a_list)
        recs = np.zeros(n, dtype=DUPLEX_DTYPE)
        sizes = (offs[0][1:] - offs[0][:-1]) + (offs[1][1:] - offs[1][:-1]) + 2
        text = C.create_string_buffer(int(sizes.sum()) + 1) if structures else None
        p64 = C.POINTER(C.c_int64)
        self._check(self.lib.mirp_set_duplex_capacity(self.h, int(capacity)), "mirp_set_duplex_capacity")
        try:
            self._check(self.lib.mirp_duplex_batch(self.h, blobs[0], offs[0].ctypes.data_as(p64), blobs[1], offs[1].ctypes.data_as(p64), n,
                                                   recs.ctypes.data_as(C.c_void_p), C.cast(text, C.c_void_p) if structures else None), "mirp_duplex_batch")
        finally:
            self.lib.mirp_set_duplex_capacity(self.h, 0)
        if not structures:
            return recs, None
        raw, at, out = text.raw, 0, []
        for sz in sizes.tolist():
            out.append(raw[at:at + sz - 1])
            at += sz
        return recs, out

    def duplex_last_stats(self):
        """{pairs, passes, evaluations} of the last duplex_batch (evaluations = loop energies evaluated)."""
        st = (C.c_int64 * 3)()
        self._check(self.lib.mirp_duplex_last_stats(self.h, st), "mirp_duplex_last_stats")
        return dict(zip(DUPLEX_STATS, list(st)))

    def ensemble(self, seqs, bpp_cutoff=None, capacity=0):
        """Partition function of whole sequences (mirp_ensemble): seqs (list of str / bytes, 1..3000 nt, A C G U/T in either
        case, anything else N), Turner-2004 with dangles 2 whatever the context's fold model.  bpp_cutoff: None, or the pairs with p >= it come
        back.  capacity: bytes of table slabs per pass (0 = the default), lowered only in tests.  -> (ENSEMBLE_DTYPE array, [bytes] of the
        centroid texts, BPP_DTYPE array ordered by (seq, i, j) or None)."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs])
        o = EnsembleOpts()
        o.bpp_cutoff, o.want_bpp, o.reserved = (0.0 if bpp_cutoff is None else float(bpp_cutoff)), int(bpp_cutoff is not None), 0
        recs = np.zeros(len(bs), dtype=ENSEMBLE_DTYPE)
        text = C.create_string_buffer(int(offs[-1]) + len(bs) + 1)
        ptr, nb = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_set_ensemble_capacity(self.h, int(capacity)), "mirp_set_ensemble_capacity")
        try:
            self._check(self.lib.mirp_ensemble(self.h, b"".join(bs), offs.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o),
                                               recs.ctypes.data_as(C.c_void_p), C.cast(text, C.c_void_p), C.byref(ptr), C.byref(nb)), "mirp_ensemble")
        finally:
            self.lib.mirp_set_ensemble_capacity(self.h, 0)
        raw, at, cen = text.raw, 0, []
        for b in bs:
            cen.append(raw[at:at + len(b)])
            at += len(b) + 1
        if bpp_cutoff is None:
            return recs, cen, None
        return recs, cen, (_copy_out(self.lib, ptr, BPP_DTYPE, nb.value) if ptr.value else np.zeros(0, dtype=BPP_DTYPE))

    def ensemble_last_stats(self):
        """{sequences, passes, cells} of the last ensemble."""
        st = (C.c_int64 * 3)()
        self._check(self.lib.mirp_ensemble_last_stats(self.h, st), "mirp_ensemble_last_stats")
        return dict(zip(ENSEMBLE_STATS, list(st)))

    def unpaired_batch(self, seqs, lo, hi, capacity=0):
        """Accessibility of intervals (mirp_unpaired_batch): for seqs[q] (str / bytes, 1..128 nt, letters as duplex_batch) and the
        1-based interval lo[q] .. hi[q], efe = -kT ln Z, efe_open = -kT ln Z over the structures that leave the interval unpaired, and upe = their
        difference, in kcal/mol.  capacity: windows per pass (0 = the default), lowered only in tests.  -> UNPAIRED_DTYPE array."""
        if not len(seqs) == len(lo) == len(hi):
            raise ValueError("unpaired_batch: %d sequences, %d lo and %d hi" % (len(seqs), len(lo), len(hi)))
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        offs = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            offs[1:] = np.cumsum([len(b) for b in bs])
        lo32, hi32 = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
        recs = np.zeros(len(bs), dtype=UNPAIRED_DTYPE)
        p32 = C.POINTER(C.c_int32)
        self._check(self.lib.mirp_set_unpaired_capacity(self.h, int(capacity)), "mirp_set_unpaired_capacity")
        try:
            self._check(self.lib.mirp_unpaired_batch(self.h, b"".join(bs), offs.ctypes.data_as(C.POINTER(C.c_int64)), lo32.ctypes.data_as(p32),
                                                     hi32.ctypes.data_as(p32), len(bs), recs.ctypes.data_as(C.c_void_p)), "mirp_unpaired_batch")
        finally:
            self.lib.mirp_set_unpaired_capacity(self.h, 0)
        return recs

    def unpaired_last_stats(self):
        """{windows, passes, cells} of the last unpaired_batch."""
        st = (C.c_int64 * 3)()
        self._check(self.lib.mirp_unpaired_last_stats(self.h, st), "mirp_unpaired_last_stats")
        return dict(zip(UNPAIRED_STATS, list(st)))

    def unpaired_lds_longest(self):
        """The longest window whose tables unpaired_batch keeps in LDS (mirp_unpaired_lds_longest); longer ones have them in device memory."""
        return int(self.lib.mirp_unpaired_lds_longest())

    def hairpin_align(self, queries, known, match=2, mismatch=3, gap_open=5, gap_extend=2, min_score=60, max_lines=0, capacity=0):
        """Gapped local alignment of every query with every known sequence (mirp_hairpin_align): queries, known (lists of str /
        bytes, 1..3000 nt, A C G U/T in either case, anything else mismatches everything).  capacity: device bytes per pass (0 = the default),
        lowered only in tests.  -> (HAIRPIN_DTYPE array of the hits with score >= min_score ordered by (query, score descending, known), at most
        max_lines per query (0 = all), [str] of their cigars: runs of = X I D, the query playing the read)."""
        blobs, offs = [], []
        for seqs in (queries, known):
            bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
            o = np.zeros(len(bs) + 1, dtype=np.int64)
            if bs:
                o[1:] = np.cumsum([len(b) for b in bs])
            blobs.append(b"".join(bs))
            offs.append(o)
        o = HairpinOpts()
        o.match, o.mismatch, o.gap_open, o.gap_extend, o.min_score, o.reserved, o.max_lines = (int(match), int(mismatch), int(gap_open), int(gap_extend),
                                                                                               int(min_score), 0, int(max_lines))
        hits, n_hits, ops, ops_off = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p()
        p64 = C.POINTER(C.c_int64)
        self._check(self.lib.mirp_set_hairpin_capacity(self.h, int(capacity)), "mirp_set_hairpin_capacity")
        try:
            self._check(self.lib.mirp_hairpin_align(self.h, blobs[0], offs[0].ctypes.data_as(p64), len(queries), blobs[1], offs[1].ctypes.data_as(p64), len(known),
                                                    C.byref(o), C.byref(hits), C.byref(n_hits), C.byref(ops), C.byref(ops_off)), "mirp_hairpin_align")
        finally:
            self.lib.mirp_set_hairpin_capacity(self.h, 0)
        n = n_hits.value
        if n == 0:
            return np.zeros(0, dtype=HAIRPIN_DTYPE), []
        at = _copy_out(self.lib, ops_off, np.int64, n + 1)
        text = _copy_out(self.lib, ops, np.uint8, int(at[-1])).tobytes()
        recs = _copy_out(self.lib, hits, HAIRPIN_DTYPE, n)
        return recs, [cigar_of(text[int(a):int(b)]) for a, b in zip(at[:-1], at[1:])]

    def hairpin_last_stats(self):
        """{queries, known, pairs, cells, hits (before the max_lines cut), passes, score_passes, trace_passes, seconds, per_query} of the last
        hairpin_align; seconds = {upload, scoring, filter + sort + cut, traceback, download}; per_query: the hits of every query before the cut."""
        st = (C.c_int64 * 8)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_hairpin_last_stats(self.h, st, sec, None), "mirp_hairpin_last_stats")
        per = np.zeros(st[0] + 1, dtype=np.int64)          # (st[0] = the queries of that call: what the library writes)
        self._check(self.lib.mirp_hairpin_last_stats(self.h, st, sec, per.ctypes.data_as(C.POINTER(C.c_int64))), "mirp_hairpin_last_stats")
        return dict(zip(HAIRPIN_STATS, list(st)), seconds=list(sec), per_query=per[:st[0]].tolist())

    def inverted_scan(self, contigs, max_span=2000, min_score=50, match=3, mismatch=4, gap=12, capacity=0):
        """Inverted repeats of every contig (mirp_inverted_scan): contigs (list of str / bytes / uint8 arrays of any length; A C G
        T/U in either case, any other byte pairs with nothing, a byte >= 0x80 is refused).  capacity: device bytes per pass (0 = the default),
        lowered only in tests.  -> (INVERTED_DTYPE array of the accepted repeats ordered by (contig, left_start, right_end), [str] of their
        structures: runs of = X L R from the outer end inwards)."""
        bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in contigs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        o = InvertedOpts()
        o.max_span, o.min_score, o.match, o.mismatch, o.gap, o.reserved = int(max_span), int(min_score), int(match), int(mismatch), int(gap), 0
        recs, n_recs, ops, ops_off = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mirp_set_inverted_capacity(self.h, int(capacity)), "mirp_set_inverted_capacity")
        try:
            self._check(self.lib.mirp_inverted_scan(self.h, b"".join(bs), off.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o), C.byref(recs),
                                                    C.byref(n_recs), C.byref(ops), C.byref(ops_off)), "mirp_inverted_scan")
        finally:
            self.lib.mirp_set_inverted_capacity(self.h, 0)
        n = n_recs.value
        if n == 0:
            return np.zeros(0, dtype=INVERTED_DTYPE), []
        at = _copy_out(self.lib, ops_off, np.int64, n + 1)
        text = _copy_out(self.lib, ops, np.uint8, int(at[-1])).tobytes()
        r = _copy_out(self.lib, recs, INVERTED_DTYPE, n)
        return r, [cigar_of(text[int(a):int(b)]) for a, b in zip(at[:-1], at[1:])]

    def inverted_last_stats(self):
        """{contigs, bases, cells, rows_above, candidates, traced, dropped_untraced, accepted, scan_passes, trace_passes, tiles, seconds} of the
        last inverted_scan; seconds = {upload, scan, candidates + sort, traceback + selection, download}."""
        st = (C.c_int64 * 12)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_inverted_last_stats(self.h, st, sec), "mirp_inverted_last_stats")
        return dict(zip(INVERTED_STATS, list(st)), seconds=list(sec))

    def nats_scan(self, seqs, seed=16, band=64, max_occ=200, min_seeds=1, match=3, mismatch=4, gap=12, min_score=200, min_length=100, capacity=0):
        """Complementary regions of every pair of transcripts a < b (mirp_nats_scan): seqs (list of str / bytes / uint8 arrays; A C
        G T/U in either case, any other byte equals nothing, a byte >= 0x80 is refused; an empty transcript and one longer than NATS_MAX_LEN are
        skipped and keep their index).  capacity: device bytes per pass (0 = the default), lowered only in tests.  -> (NATS_DTYPE array of the
        regions ordered by (a, b, a_start, b_start), [str] of their cigars: runs of = X I D in a's 5'->3' order)."""
        bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        o = NatsOpts()
        (o.seed, o.band, o.max_occ, o.min_seeds, o.match, o.mismatch, o.gap, o.min_score, o.min_length, o.reserved) = (
            int(seed), int(band), int(max_occ), int(min_seeds), int(match), int(mismatch), int(gap), int(min_score), int(min_length), 0)
        recs, n_recs, ops, ops_off = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mirp_set_nats_capacity(self.h, int(capacity)), "mirp_set_nats_capacity")
        try:
            self._check(self.lib.mirp_nats_scan(self.h, b"".join(bs), off.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o), C.byref(recs),
                                                C.byref(n_recs), C.byref(ops), C.byref(ops_off)), "mirp_nats_scan")
        finally:
            self.lib.mirp_set_nats_capacity(self.h, 0)
        n = n_recs.value
        if n == 0:
            return np.zeros(0, dtype=NATS_DTYPE), []
        at = _copy_out(self.lib, ops_off, np.int64, n + 1)
        text = _copy_out(self.lib, ops, np.uint8, int(at[-1])).tobytes()
        r = _copy_out(self.lib, recs, NATS_DTYPE, n)
        return r, [cigar_of(text[int(a):int(b)]) for a, b in zip(at[:-1], at[1:])]

    def nats_last_stats(self):
        """{transcripts, skipped, bases, kmers_ignored, seed_hits, candidates, kept_candidates, cells, above, traced, regions, pairs, join_passes,
        scan_launches, trace_passes, seconds} of the last nats_scan; seconds = {upload + keys, sort + runs, join + candidates, band scan,
        traceback, selection}."""
        st = (C.c_int64 * 16)()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_nats_last_stats(self.h, st, sec), "mirp_nats_last_stats")
        return dict(zip(NATS_STATS, list(st)), seconds=list(sec))

    def homolog_scan(self, queries, max_mismatches=1, precursor_len=300, max_placements=100, keys=0, chunk=0, fold_lines=0, eval_caps=(0, 0, 0)):
        """Homologs of known mature miRNAs in the genome of align_index (mirp_homolog_scan).  queries: distinct sequences (str /
        bytes) of 18..26 letters A C G T/U.  keys, chunk, fold_lines, eval_caps (pieces, structures, staged lines): the capacities of
        mirp_set_homolog_capacity, lowered only in tests.  -> (HOMOLOG_DTYPE array of the loci ordered by (contig, fold_s, strand, mat_s, mat_e),
        the text bytes (per locus at text_off: the window's letters on its strand, then the dot-bracket structure), int32 array [n, 2] of the
        (query, mismatches) pairs the loci's also_off / n_also point into)."""
        bs = [q.encode() if isinstance(q, str) else bytes(q) for q in queries]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        o = HomologOpts()
        o.max_mismatches, o.precursor_len, o.max_placements, o.reserved = int(max_mismatches), int(precursor_len), int(max_placements), 0
        recs, n_recs, text, also = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_void_p()
        self._check(self.lib.mirp_set_homolog_capacity(self.h, int(keys), int(chunk), int(fold_lines), *[int(x) for x in eval_caps]), "mirp_set_homolog_capacity")
        try:
            self._check(self.lib.mirp_homolog_scan(self.h, b"".join(bs), off.ctypes.data_as(C.POINTER(C.c_int64)), len(bs), C.byref(o), C.byref(recs),
                                                   C.byref(n_recs), C.byref(text), C.byref(also)), "mirp_homolog_scan")
        finally:
            self.lib.mirp_set_homolog_capacity(self.h, 0, 0, 0, 0, 0, 0)
        n = n_recs.value
        if n == 0:
            return np.zeros(0, dtype=HOMOLOG_DTYPE), b"", np.zeros((0, 2), dtype=np.int32)
        r = _copy_out(self.lib, recs, HOMOLOG_DTYPE, n)
        t = _copy_out(self.lib, text, np.uint8, int((r["win_e"].astype(np.int64) - r["win_s"] + r["ss_len"]).sum())).tobytes()
        a = _copy_out(self.lib, also, np.int32, 2 * int(r["n_also"].sum())).reshape(-1, 2)
        return r, t, a

    def align_contigs(self):
        """([names as str], int64 array of lengths) of the contigs of align_index in reference order (mirp_homolog_contigs)."""
        names, size, lens, n = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int32()
        self._check(self.lib.mirp_homolog_contigs(self.h, C.byref(names), C.byref(size), C.byref(lens), C.byref(n)), "mirp_homolog_contigs")
        ln = _copy_out(self.lib, lens, np.int64, n.value)
        blob = _copy_out(self.lib, names, np.uint8, size.value).tobytes().decode("latin-1")
        return blob.split("\0")[:-1], ln

    def homolog_last_stats(self):
        """{queries, repeat_like, placements, passing, loci, scan_passes, chunks, folds, eval_reruns, eval_global_text (launches of the evaluation
        kernel with the staged text in global memory), fail_codes, no_structure, seconds} of the last homolog_scan; fail_codes[k]:
        placements without a passing structure whose structure of lowest normalised energy has get_maturestar_info code k (index 0 unused);
        seconds = {scan, windows, fold, evaluation + download, merge}."""
        st = (C.c_int64 * 24)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_homolog_last_stats(self.h, st, sec), "mirp_homolog_last_stats")
        return dict(zip(HOMOLOG_STATS, list(st)[:10]), fail_codes=[0] + list(st)[11:23], no_structure=int(st[23]), seconds=list(sec))

    def last_jobs_per_slot(self, family):
        """(launches, the largest ceil(jobs / slots) over them) of a wave-per-job kernel family in the last call that can launch it
        (mirp_last_jobs_per_slot): family 0 = two-strand fold (duplex_batch, target_scan), 1 = accessibility (unpaired_batch, target_scan),
        2 = hairpin scoring (hairpin_align; the largest chunk of queries), 3 = homolog evaluation (homolog_scan), 4 = the filter kernel (predict_batch, predict_batch_reasons, predict, predict_reasons; windows per
        workgroup, re-runs of windows over a capacity included), 5 = the count kernel of the locus scan (locus_scan; (locus, chunk) jobs per wave), 6 = the sum kernel of the exact test (diffexp; (feature, chunk)
        jobs per wave), 7 = the overlap kernel of the signature scan (signature_scan; (locus, chunk of U entries) jobs per wave), 8 = the band scan of
        nats_scan (candidates per wave)."""
        out = (C.c_int64 * 2)()
        self._check(self.lib.mirp_last_jobs_per_slot(self.h, int(family), out), "mirp_last_jobs_per_slot")
        return int(out[0]), int(out[1])

    def phase_scan(self, length, cycles, kmin, min_phased=3, min_depth=1):
        """Phased siRNA windows on this context's resident alignments (mirp_phase_scan).  kmin: the int32 table of the smallest
        phased count that passes at each n = 0 .. 2 * cycles * length.  -> (PHASE_WINDOW_DTYPE array of the passing windows in (tid, start) order,
        {records, units, anchors})."""
        o = PhaseOpts()
        o.length, o.cycles, o.min_phased, o.min_depth = int(length), int(cycles), int(min_phased), int(min_depth)
        km = np.ascontiguousarray(kmin, dtype=np.int32)
        if len(km) != 2 * int(cycles) * int(length) + 1:
            raise ValueError("phase_scan: kmin needs 2 * cycles * length + 1 entries")
        ptr, nw = C.c_void_p(), C.c_int64()
        st = (C.c_int64 * 3)()
        self._check(self.lib.mirp_phase_scan(self.h, C.byref(o), km.ctypes.data, C.byref(ptr), C.byref(nw), st), "mirp_phase_scan")
        return _copy_out(self.lib, ptr, PHASE_WINDOW_DTYPE, nw.value), dict(zip(("records", "units", "anchors"), list(st)))

    def trigger_scan(self, mirna_path, genome_paths, loci, length, cycles, kmin, min_phased=3, min_depth=1, max_half_score=8, drift=0):
        """miRNA triggers of PHAS loci on this context's resident alignments (mirp_trigger_scan).  loci: TRIGGER_LOCUS_DTYPE, the
        intervals already widened and clipped; kmin as for phase_scan; max_half_score = 2 x the -s score.  -> (TRIGGER_DTYPE array in output order,
        int64 sites per locus, {mirnas, interval_bases, sites, windows, records, units, seconds}); seconds = {parse + pack, upload, site scan + sort,
        units, windows + download}."""
        loci = np.ascontiguousarray(loci, dtype=TRIGGER_LOCUS_DTYPE)
        o = TriggerOpts()
        o.length, o.cycles, o.min_phased, o.min_depth, o.max_half_score, o.drift = (int(length), int(cycles), int(min_phased), int(min_depth),
                                                                                  int(max_half_score), int(drift))
        km = np.ascontiguousarray(kmin, dtype=np.int32)
        if len(km) != 2 * int(cycles) * int(length) + 1:
            raise ValueError("trigger_scan: kmin needs 2 * cycles * length + 1 entries")
        paths = [genome_paths] if isinstance(genome_paths, (str, bytes, os.PathLike)) else list(genome_paths)
        arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
        counts = np.zeros(max(len(loci), 1), dtype=np.int64)
        ptr, nt = C.c_void_p(), C.c_int64()
        st = (C.c_int64 * 6)()
        sec = (C.c_double * 5)()
        self._check(self.lib.mirp_trigger_scan(self.h, os.fsencode(mirna_path), arr, len(paths), loci.ctypes.data, len(loci), C.byref(o), km.ctypes.data,
                                               C.byref(ptr), C.byref(nt), counts.ctypes.data, st, sec), "mirp_trigger_scan")
        return _copy_out(self.lib, ptr, TRIGGER_DTYPE, nt.value), counts[:len(loci)], dict(zip(TRIGGER_STATS, list(st)), seconds=list(sec))

    def cluster_scan(self, threshold, pad, contig_lens, n_samples):
        """Small-RNA clusters on this context's resident alignments (mirp_cluster_scan).  threshold: the integer coverage T;
        contig_lens: LN per contig.  -> (CLUSTER_DTYPE array in (tid, start) order, int64 [clusters, n_samples] depth per sample,
        {records, total, islands, clusters, assigned})."""
        lens = np.ascontiguousarray(contig_lens, dtype=np.int64)
        o = ClusterOpts()
        o.threshold, o.pad, o.contig_len, o.n_contigs, o.n_samples = int(threshold), int(pad), lens.ctypes.data, len(lens), int(n_samples)
        ptr, cnt, nc = C.c_void_p(), C.c_void_p(), C.c_int64()
        st = (C.c_int64 * 5)()
        self._check(self.lib.mirp_cluster_scan(self.h, C.byref(o), C.byref(ptr), C.byref(nc), C.byref(cnt), st), "mirp_cluster_scan")
        clusters = _copy_out(self.lib, ptr, CLUSTER_DTYPE, nc.value)
        counts = _copy_out(self.lib, cnt, np.dtype("<i8"), nc.value * int(n_samples)).reshape(nc.value, int(n_samples))
        return clusters, counts, dict(zip(CLUSTER_STATS, list(st)))

    def locus_scan(self, loci, contig_lens, n_samples, stranded=False):
        """Reads on given loci on this context's resident alignments (mirp_locus_scan).  loci: LOCUS_DTYPE, which may overlap, nest
        and repeat; contig_lens: LN per contig.  -> (CLUSTER_DTYPE array, one row per locus in input order, int64 [loci, n_samples] depth per
        sample, {records, loci, jobs, pairs, max_len})."""
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        lens = np.ascontiguousarray(contig_lens, dtype=np.int64)
        o = LocusOpts()
        o.contig_len, o.n_contigs, o.n_samples, o.stranded, o.reserved = lens.ctypes.data, len(lens), int(n_samples), int(bool(stranded)), 0
        ptr, cnt = C.c_void_p(), C.c_void_p()
        st = (C.c_int64 * 5)()
        self._check(self.lib.mirp_locus_scan(self.h, loci.ctypes.data, len(loci), C.byref(o), C.byref(ptr), C.byref(cnt), st), "mirp_locus_scan")
        nl, S = len(loci), int(n_samples)
        rows = _copy_out(self.lib, ptr, CLUSTER_DTYPE, nl)
        counts = _copy_out(self.lib, cnt, np.dtype("<i8"), nl * S).reshape(nl, S)
        return rows, counts, dict(zip(LOCUS_STATS, list(st)))

    def signature_scan(self, loci, contig_lens, min_len=20, max_len=25, max_overlap=30, overhang=2, min_reads=5):
        """siRNA duplexes and the 5' overlap signature on given loci, on this context's resident alignments (mirp_signature_scan).
        loci: LOCUS_DTYPE (the strand is ignored), which may overlap, nest and repeat; contig_lens: LN per contig.  -> (SIGNATURE_ROW_DTYPE array,
        one row per locus in input order, int64 [loci, max_overlap] H with column k - 1 = overlap k, DUPLEX_SITE_DTYPE array of the duplexes with
        min(plus_reads, minus_reads) >= min_reads in (locus, pos, len) order, {records, kept, u_entries, v_entries, jobs, sites})."""
        loci = np.ascontiguousarray(loci, dtype=LOCUS_DTYPE)
        lens = np.ascontiguousarray(contig_lens, dtype=np.int64)
        o = SignatureOpts()
        o.contig_len, o.n_contigs, o.min_len, o.max_len, o.max_overlap, o.overhang, o.reserved, o.min_reads = (
            lens.ctypes.data, len(lens), int(min_len), int(max_len), int(max_overlap), int(overhang), 0, int(min_reads))
        rows, hp, sp, ns = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        st = (C.c_int64 * 6)()
        self._check(self.lib.mirp_signature_scan(self.h, loci.ctypes.data, len(loci), C.byref(o), C.byref(rows), C.byref(hp), C.byref(sp), C.byref(ns),
                                                 st), "mirp_signature_scan")
        nl, K = len(loci), int(max_overlap)
        out = _copy_out(self.lib, rows, SIGNATURE_ROW_DTYPE, nl)
        H = _copy_out(self.lib, hp, np.dtype("<i8"), nl * K).reshape(nl, K)
        sites = _copy_out(self.lib, sp, DUPLEX_SITE_DTYPE, ns.value)
        return out, H, sites, dict(zip(SIGNATURE_STATS, list(st)))

    def diffexp(self, counts, size_factors, groups, mode="max", phi=0.0, min_mean=10.0, pseudo=0.5):
        """The exact negative-binomial test between two groups of samples (mirp_diffexp).  counts: [features, samples] whole
        numbers, the used samples only; size_factors: one per sample; groups: 0 (A) or 1 (B) per sample; mode: one of DIFFEXP_MODES or its
        index, `phi` the dispersion of mode "fixed".  -> (DIFFEXP_DTYPE array, one row per feature in input order, p = -1 where untested,
        {features, tested, jobs, terms, phi_c})."""
        counts = np.ascontiguousarray(counts, dtype=np.uint64)
        if counts.ndim != 2:
            raise ValueError("diffexp: counts must be [features, samples]")
        sf = np.ascontiguousarray(size_factors, dtype=np.float64)
        grp = np.ascontiguousarray(groups, dtype=np.uint8)
        if len(sf) != counts.shape[1] or len(grp) != counts.shape[1]:
            raise ValueError("diffexp: size_factors and groups need one value per sample")
        o = DiffexpOpts()
        o.size_factor, o.group, o.n_samples = sf.ctypes.data, grp.ctypes.data, counts.shape[1]
        o.mode = DIFFEXP_MODES.index(mode) if isinstance(mode, str) else int(mode)
        o.phi, o.min_mean, o.pseudo = float(phi), float(min_mean), float(pseudo)
        ptr = C.c_void_p()
        st = (C.c_int64 * 5)()
        self._check(self.lib.mirp_diffexp(self.h, counts.ctypes.data if counts.size else None, counts.shape[0], C.byref(o), C.byref(ptr), st),
                    "mirp_diffexp")
        rows = _copy_out(self.lib, ptr, DIFFEXP_DTYPE, counts.shape[0])
        stats = dict(zip(DIFFEXP_STATS[:4], list(st)[:4]))
        stats["phi_c"] = float(np.array([st[4]], dtype=np.int64).view(np.float64)[0])
        return rows, stats

    def isomir_scan(self, alns, tails, loci, max5, max3, n_samples):
        """isomiR counts (mirp_isomir_scan).  alns: ALN_DTYPE records with pos = POS and len = the templated length; tails: their uint32
        tail codes; loci: ISO_LOCUS_DTYPE in file order.  -> (ISOMIR_DTYPE array in (locus, d5, d3, tail) order, ISO_SUM_DTYPE per locus, int64
        [loci, n_samples], int64 [isomiRs, n_samples], {records, assigned, depth, isomirs})."""
        alns = np.ascontiguousarray(alns)
        assert alns.dtype.itemsize == 16
        tails = np.ascontiguousarray(tails, dtype="<u4")
        loci = np.ascontiguousarray(loci, dtype=ISO_LOCUS_DTYPE)
        if len(tails) != len(alns):
            raise ValueError("isomir_scan: alns and tails differ in length")
        o = IsomirOpts()
        o.max5, o.max3, o.n_samples, o.reserved = int(max5), int(max3), int(n_samples), 0
        iso, sums, lc, ic, ni = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
        st = (C.c_int64 * 4)()
        self._check(self.lib.mirp_isomir_scan(self.h, alns.ctypes.data, tails.ctypes.data, len(alns), loci.ctypes.data, len(loci), C.byref(o),
                                              C.byref(iso), C.byref(ni), C.byref(sums), C.byref(lc), C.byref(ic), st), "mirp_isomir_scan")
        S, nl = int(n_samples), len(loci)
        return (_copy_out(self.lib, iso, ISOMIR_DTYPE, ni.value), _copy_out(self.lib, sums, ISO_SUM_DTYPE, nl),
                _copy_out(self.lib, lc, np.dtype("<i8"), nl * S).reshape(nl, S), _copy_out(self.lib, ic, np.dtype("<i8"), ni.value * S).reshape(ni.value, S),
                dict(zip(ISOMIR_STATS, list(st))))

    def degradome_scan(self, mirna_path, transcripts_path, out_path, contig_names, contig_lens, max_half_score=8, cleavage_site=False, max_category=4,
                       alpha=1.0):
        """Degradome (PARE) evidence of miRNA-guided cleavage on this context's resident alignments (mirp_degradome_scan): writes the TSV
        to out_path.  contig_names / contig_lens: the @SQ lines the records' tids index.  max_half_score = 2 x the -s score.  -> {mirnas, transcripts,
        bases, records, sense, minus, units, c0 .. c4, evaluations, hits, passes, seconds}; seconds = {parse, upload, units + categories, site counts,
        anchored counts, key passes + sort + write}."""
        lens = np.ascontiguousarray(contig_lens, dtype=np.int64)
        if len(lens) != len(contig_names):
            raise ValueError("degradome_scan: contig_names and contig_lens differ in length")
        o = DegradomeOpts()
        o.max_half_score, o.cleavage_site, o.max_category, o.n_contigs, o.alpha = int(max_half_score), int(bool(cleavage_site)), int(max_category), len(lens), float(alpha)
        blob = C.create_string_buffer(b"".join((n.encode() if isinstance(n, str) else bytes(n)) + b"\0" for n in contig_names) + b"\0")
        o.contig_names = C.cast(blob, C.c_char_p)
        o.contig_len = lens.ctypes.data if len(lens) else None
        st = (C.c_int64 * 15)()
        sec = (C.c_double * 6)()
        self._check(self.lib.mirp_degradome_scan(self.h, os.fsencode(mirna_path), os.fsencode(transcripts_path), C.byref(o), os.fsencode(out_path), st, sec),
                    "mirp_degradome_scan")
        return dict(zip(DEGRADOME_STATS, list(st)), seconds=list(sec))

    def fold_batch(self, seqs, span, max_lines=96):
        """RNALfold -L replacement. seqs: list of str/bytes. Returns a list (per sequence) of
        dicts {lines: [(ss, energy, start), ...] (printed only), mfe, status}."""
        raw = self.fold_batch_raw(seqs, span, max_lines)
        out = []
        for w in range(len(seqs)):
            ls = []
            for k in range(min(int(raw["n_lines"][w]), max_lines)):      # a window over the capacity (status 1) reports the count it needs
                ln = raw["lines"][w, k]
                if not ln["printed"]:
                    continue
                ls.append((raw["ss"][w, k, :int(ln["len"])].tobytes().decode(), int(ln["energy"]), int(ln["start"])))
            out.append({"lines": ls, "mfe": int(raw["mfe"][w]), "status": int(raw["status"][w])})
        return out

    def fold_batch_summary(self, blob, offsets, span, max_lines=96):
        """Folds the sequences blob[offsets[k]:offsets[k+1]] and returns only (n_lines, mfe, status) per sequence: nothing of the structure text
        is copied back (mirp_fold_batch_summary).  blob: bytes / uint8 array, offsets: int64 array of n + 1 entries."""
        blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offs) - 1
        vp = C.c_void_p
        nl, mfe, st = vp(), vp(), vp()
        self._check(self.lib.mirp_fold_batch_summary(self.h, C.cast(blob.ctypes.data, C.c_char_p), offs.ctypes.data_as(C.POINTER(C.c_int64)), n, int(span),
                                                     int(max_lines), C.byref(nl), C.byref(mfe), C.byref(st)), "mirp_fold_batch_summary")
        return _copy_out(self.lib, nl, np.int32, n), _copy_out(self.lib, mfe, np.int32, n), _copy_out(self.lib, st, np.int32, n)

    def fold_batch_raw(self, seqs, span, max_lines=96):
        """As fold_batch but returns the C-ABI arrays: lines[n,max_lines], ss[n,max_lines,stride], n_lines, mfe, status."""
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        n = len(bs)
        offs = np.zeros(n + 1, dtype=np.int64)
        if n:
            offs[1:] = np.cumsum([len(b) for b in bs])
        blob = b"".join(bs)
        vp = C.c_void_p
        lines, ss, nl, mfe, st = vp(), vp(), vp(), vp(), vp()
        stride = C.c_int32()
        rc = self.lib.mirp_fold_batch(self.h, blob, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, int(span), int(max_lines),
                                      C.byref(lines), C.byref(ss), C.byref(stride), C.byref(nl), C.byref(mfe), C.byref(st))
        self._check(rc, "mirp_fold_batch")
        stride = stride.value
        a_lines = _copy_out(self.lib, lines, FOLD_LINE_DTYPE, n * max_lines).reshape(n, max_lines)
        a_ss = _copy_out(self.lib, ss, np.uint8, n * max_lines * stride).reshape(n, max_lines, stride)
        a_nl = _copy_out(self.lib, nl, np.int32, n)
        a_mfe = _copy_out(self.lib, mfe, np.int32, n)
        a_st = _copy_out(self.lib, st, np.int32, n)
        return {"lines": a_lines, "ss": a_ss, "stride": stride, "max_lines": max_lines, "n_lines": a_nl, "mfe": a_mfe, "status": a_st}

    def predict_batch(self, windows, matures, alns, fold_raw, params):
        """filter_next_loci/check_loci replacement. windows/matures/alns: record arrays (records.py dtypes);
        fold_raw: output of fold_batch_raw for the same windows; params: (n_samples, min_mature_len, max_mature_len,
        allow_3nt, allow_no_star, minlen).  Returns (mirnas[n, MAX_MIRNA_PER_WINDOW], n_mirnas[n], status[n])."""
        from . import records
        windows = np.ascontiguousarray(windows, dtype=records.WINDOW_DTYPE)
        matures = np.ascontiguousarray(matures, dtype=records.MATURE_DTYPE)
        alns = np.ascontiguousarray(alns)
        lines = np.ascontiguousarray(fold_raw["lines"])
        ss = np.ascontiguousarray(fold_raw["ss"])
        nl = np.ascontiguousarray(fold_raw["n_lines"], dtype=np.int32)
        n = len(windows)
        pp = (C.c_int32 * 6)(*[int(x) for x in params])
        vp = C.c_void_p
        o, no, st = vp(), vp(), vp()
        rc = self.lib.mirp_predict_batch(self.h, windows.ctypes.data, n, matures.ctypes.data, len(matures), alns.ctypes.data, len(alns),
                                         lines.ctypes.data, ss.ctypes.data, int(fold_raw["stride"]), int(fold_raw["max_lines"]),
                                         nl.ctypes.data, pp, C.byref(o), C.byref(no), C.byref(st))
        self._check(rc, "mirp_predict_batch")
        a_o = _copy_out(self.lib, o, records.MIRNA_DTYPE, n * records.MAX_MIRNA_PER_WINDOW).reshape(n, records.MAX_MIRNA_PER_WINDOW)
        return a_o, _copy_out(self.lib, no, np.int32, n), _copy_out(self.lib, st, np.int32, n)

    def predict_batch_reasons(self, windows, matures, alns, fold_raw, params):
        """predict_batch plus the -d records (mirp_predict_batch_reasons): -> (mirnas, n_mirnas, status, reasons[n_records, stride]); the layout
        of a record is documented at mirp_predict_reasons in include/mirprefer.h."""
        from . import records
        windows = np.ascontiguousarray(windows, dtype=records.WINDOW_DTYPE)
        matures = np.ascontiguousarray(matures, dtype=records.MATURE_DTYPE)
        alns = np.ascontiguousarray(alns)
        lines = np.ascontiguousarray(fold_raw["lines"])
        ss = np.ascontiguousarray(fold_raw["ss"])
        nl = np.ascontiguousarray(fold_raw["n_lines"], dtype=np.int32)
        n = len(windows)
        pp = (C.c_int32 * 6)(*[int(x) for x in params])
        vp = C.c_void_p
        o, no, st, rr = vp(), vp(), vp(), vp()
        nr, rs = C.c_int64(), C.c_int32()
        rc = self.lib.mirp_predict_batch_reasons(self.h, windows.ctypes.data, n, matures.ctypes.data, len(matures), alns.ctypes.data if len(alns) else None, len(alns),
                                                 lines.ctypes.data, ss.ctypes.data, int(fold_raw["stride"]), int(fold_raw["max_lines"]),
                                                 nl.ctypes.data, pp, C.byref(o), C.byref(no), C.byref(st), C.byref(rr), C.byref(nr), C.byref(rs))
        self._check(rc, "mirp_predict_batch_reasons")
        a_o = _copy_out(self.lib, o, records.MIRNA_DTYPE, n * records.MAX_MIRNA_PER_WINDOW).reshape(n, records.MAX_MIRNA_PER_WINDOW)
        rec = _copy_out(self.lib, rr, np.int32, nr.value * rs.value).reshape(nr.value, max(rs.value, 1)) if rr.value else np.zeros((0, max(rs.value, 1)), np.int32)
        return a_o, _copy_out(self.lib, no, np.int32, n), _copy_out(self.lib, st, np.int32, n), rec

    # ---- device-resident pipeline -------------------------------------------------------------
    def load_genome(self, contigs):
        """contigs: list of (name, uint8 array) in @SQ order."""
        lens = np.array([len(s) for _, s in contigs], dtype=np.int64)
        arrs = [s for _, s in contigs]
        base = arrs[0].base if arrs and isinstance(arrs[0], np.ndarray) else None
        if (isinstance(base, np.ndarray) and base.ndim == 1 and base.dtype == np.uint8 and base.flags.c_contiguous and len(base) == int(lens.sum()) and
                all(isinstance(a, np.ndarray) and a.dtype == np.uint8 for a in arrs) and arrs[0].ctypes.data == base.ctypes.data and
                all(a.ctypes.data + len(a) == b.ctypes.data for a, b in zip(arrs, arrs[1:]))):
            blob = base          # the contigs are consecutive slices of one buffer (capi.read_fasta): upload it as it is
        else:
            blob = np.concatenate(arrs) if contigs else np.zeros(0, np.uint8)
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self.lib.mirp_load_genome(self.h, len(contigs), lens.ctypes.data, blob.ctypes.data), "mirp_load_genome")

    def load_alignments(self, alns):
        alns = np.ascontiguousarray(alns)
        assert alns.dtype.itemsize == 16
        self._check(self.lib.mirp_load_alignments(self.h, alns.ctypes.data, len(alns)), "mirp_load_alignments")

    def load_coverage_segments(self, segs):
        """Coverage segments of gapped alignments (see mirp_load_coverage_segments); call after load_alignments."""
        segs = np.ascontiguousarray(segs)
        assert segs.dtype.itemsize == 16
        self._check(self.lib.mirp_load_coverage_segments(self.h, segs.ctypes.data, len(segs)), "mirp_load_coverage_segments")

    def ingest_sams(self, paths, regions=None, n_threads=0):
        """SAM files -> sorted records with the device doing the record work (mirp_ingest_sams_gpu): host threads tokenize, the GPU filters by
        the keep regions [(tid, start0, end0), ...] like `samtools view -L` and sorts stably by (tid, pos).  The records stay resident as this
        context's alignments.  -> (contig_names, contig_lens, sample_names, alns, segs, seconds{tokenize, upload_filter, sort, download})."""
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        nreg = len(regions) if regions else 0
        reg = (Region * max(nreg, 1))()
        for k in range(nreg):
            reg[k].tid, reg[k].start, reg[k].end = int(regions[k][0]), int(regions[k][1]), int(regions[k][2])
        d = SamData()
        sec = (C.c_double * 4)()
        import time
        t0 = time.time()
        rc = self.lib.mirp_ingest_sams_gpu(self.h, arr, len(paths), int(n_threads), C.cast(reg, C.c_void_p), nreg, C.byref(d), sec)
        t1 = time.time()
        if rc != 0:
            raise ValueError(self.lib.mirp_last_error(self.h).decode())
        cn, lens, sn, alns, segs = _unpack_sam_data(self.lib, d)
        # native_other_s: what the library call spends outside its four phases (opening / mapping the files, the host buffers of the result);
        # host_copy_s: the records copied out of the library's buffer into numpy arrays and the buffer released
        return cn, lens, sn, alns, segs, {"tokenize_s": sec[0], "upload_filter_s": sec[1], "sort_s": sec[2], "download_s": sec[3],
                                          "native_other_s": max(0.0, (t1 - t0) - sum(sec)), "host_copy_s": time.time() - t1}

    def ingest_tokenized(self, paths, regions=None):
        """The device half of ingest_sams for files whose tokenizer run the CLI started before its heavy imports (early.start_ingest): keep-region filter +
        stable radix sort (mirp_ingest_tokenized_gpu).  Same return as ingest_sams."""
        got = early.take_ingest(paths)
        if got is None:
            raise MirpError("ingest_tokenized: no tokenizer run was started for these files")
        rc, tok, msg = got
        if rc != 0:
            raise ValueError(msg)
        nreg = len(regions) if regions else 0
        reg = (Region * max(nreg, 1))()
        for k in range(nreg):
            reg[k].tid, reg[k].start, reg[k].end = int(regions[k][0]), int(regions[k][1]), int(regions[k][2])
        d = SamData()
        sec = (C.c_double * 4)()
        fn = self.lib.mirp_ingest_tokenized_gpu
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SamData), C.POINTER(C.c_double)]
        fn.restype = C.c_int
        if fn(self.h, tok, C.cast(reg, C.c_void_p), nreg, C.byref(d), sec) != 0:
            raise ValueError(self.lib.mirp_last_error(self.h).decode())
        cn, lens, sn, alns, segs = _unpack_sam_data(self.lib, d)
        return cn, lens, sn, alns, segs, {"tokenize_s": 0.0, "upload_filter_s": sec[1], "sort_s": sec[2], "download_s": sec[3]}

    def ingest_sams_shard(self, paths, owner_of_tid, regions=None, n_threads=0):
        """Sharded ingest (mirp_ingest_sams_shard): this rank tokenizes its byte range of every file, records travel to the rank that owns their
        contig over RCCL (dist_init first), this rank filters / sorts / keeps its own.  Same return as ingest_sams, records of this rank's contigs."""
        arr = (C.c_char_p * len(paths))(*[str(p).encode() for p in paths])
        nreg = len(regions) if regions else 0
        reg = (Region * max(nreg, 1))()
        for k in range(nreg):
            reg[k].tid, reg[k].start, reg[k].end = int(regions[k][0]), int(regions[k][1]), int(regions[k][2])
        own = np.ascontiguousarray(owner_of_tid, dtype=np.int32) if owner_of_tid is not None else None
        d = SamData()
        sec = (C.c_double * 4)()
        rc = self.lib.mirp_ingest_sams_shard(self.h, arr, len(paths), int(n_threads), C.cast(reg, C.c_void_p), nreg,
                                             own.ctypes.data if own is not None else None, C.byref(d), sec)
        if rc != 0:
            raise ValueError(self.lib.mirp_last_error(self.h).decode())
        cn, lens, sn, alns, segs = _unpack_sam_data(self.lib, d)
        return cn, lens, sn, alns, segs, {"tokenize_s": sec[0], "exchange_upload_filter_s": sec[1], "sort_s": sec[2], "download_s": sec[3]}

    # ---- multi-GPU: RCCL communicator of this context (one process per GPU) -------------------
    def dist_unique_id(self):
        """128 bytes of ncclGetUniqueId: rank 0 calls this and hands the bytes to every rank's dist_init."""
        buf = (C.c_uint8 * 128)()
        if self.lib.mirp_dist_unique_id(buf) != 0:
            raise MirpError("mirp_dist_unique_id failed (librccl.so.1 not loadable?)")
        return bytes(buf)

    def dist_init(self, unique_id, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.lib.mirp_dist_init(self.h, buf, int(rank), int(world)), "mirp_dist_init")

    def dist_init_local(self, directory, rank, world):
        """Ranks that share one GPU: exchanges staged through files in `directory` (mirp_dist_init_local)."""
        self._check(self.lib.mirp_dist_init_local(self.h, str(directory).encode(), int(rank), int(world)), "mirp_dist_init_local")

    def dist_finalize(self):
        self._check(self.lib.mirp_dist_finalize(self.h), "mirp_dist_finalize")

    def dist_world(self):
        return int(self.lib.mirp_dist_world(self.h))

    def dist_comm_info(self):
        """{ncclCommCount, ncclCommUserRank, ncclCommCuDevice} of the context's RCCL communicator; -1s without one."""
        v = (C.c_int32 * 3)()
        self._check(self.lib.mirp_dist_comm_info(self.h, v), "mirp_dist_comm_info")
        return {"comm_count": int(v[0]), "comm_rank": int(v[1]), "comm_device": int(v[2])}

    def dist_barrier(self):
        self._check(self.lib.mirp_dist_barrier(self.h), "mirp_dist_barrier")

    def dist_allreduce_sum(self, values):
        v = np.ascontiguousarray(values, dtype=np.int64).copy()
        self._check(self.lib.mirp_dist_allreduce_sum(self.h, v.ctypes.data, len(v)), "mirp_dist_allreduce_sum")
        return v

    def gather_loci(self, dst=0):
        """The result of the last predict() of every rank on rank dst (rank order): {"result": MIRNA records, "ss": [str]}; empty elsewhere."""
        from . import records
        r, t = C.c_void_p(), C.c_void_p()
        n, stride = C.c_int64(), C.c_int32()
        self._check(self.lib.mirp_gather_loci(self.h, int(dst), C.byref(r), C.byref(n), C.byref(t), C.byref(stride)), "mirp_gather_loci")
        res = _copy_out(self.lib, r, records.MIRNA_DTYPE, n.value) if r.value else np.zeros(0, dtype=records.MIRNA_DTYPE)
        txt = _copy_out(self.lib, t, np.uint8, n.value * stride.value).reshape(n.value, stride.value) if t.value else np.zeros((0, max(stride.value, 1)), np.uint8)
        ss = [txt[k, :res[k]["ss_len"]].tobytes().decode() for k in range(n.value)]
        return {"result": res, "ss": ss}

    def gather_records(self, rec, dst=0):
        """Fixed-size records (a C-contiguous numpy array, first axis = records) of every rank on rank dst, in rank order; None elsewhere."""
        rec = np.ascontiguousarray(rec)
        rb = int(rec.dtype.itemsize * (rec.size // max(len(rec), 1))) if len(rec) else int(rec.dtype.itemsize * int(np.prod(rec.shape[1:], dtype=np.int64)))
        o, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_gather_records(self.h, rec.ctypes.data if len(rec) else None, len(rec), max(rb, 1), int(dst), C.byref(o), C.byref(n)),
                    "mirp_gather_records")
        if not o.value:
            return None
        flat = _copy_out(self.lib, o, np.uint8, n.value * max(rb, 1))
        return flat.view(rec.dtype).reshape((n.value,) + rec.shape[1:])

    def candidate(self, cutoff, max_gap, precursor_len, contig_order, min_peak_len=19):
        pp = (C.c_int32 * 4)(int(cutoff), int(min_peak_len), int(max_gap), int(precursor_len))
        order = np.ascontiguousarray(contig_order, dtype=np.int32)
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.mirp_candidate(self.h, pp, order.ctypes.data, C.byref(a), C.byref(b), C.byref(c)), "mirp_candidate")
        self._n_windows = c.value
        return a.value, b.value, c.value

    def get_depth(self):
        from . import records
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_get_depth(self.h, C.byref(p), C.byref(n)), "mirp_get_depth")
        return _copy_out(self.lib, p, records.DEPTH_DTYPE, n.value)

    def get_peaks(self):
        from . import records
        p, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_get_peaks(self.h, C.byref(p), C.byref(n)), "mirp_get_peaks")
        return _copy_out(self.lib, p, records.PEAK_DTYPE, n.value)

    def get_loci(self):
        from . import records
        p, n, q, m = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_get_loci(self.h, C.byref(p), C.byref(n), C.byref(q), C.byref(m)), "mirp_get_loci")
        return _copy_out(self.lib, p, records.LOCUS_DTYPE, n.value), _copy_out(self.lib, q, records.PEAK_DTYPE, m.value)

    def get_windows(self):
        from . import records
        vp = C.c_void_p
        w, nw, pk, npk, mt, nmt, sq, nsq = vp(), C.c_int64(), vp(), C.c_int64(), vp(), C.c_int64(), vp(), C.c_int64()
        self._check(self.lib.mirp_get_windows(self.h, C.byref(w), C.byref(nw), C.byref(pk), C.byref(npk), C.byref(mt), C.byref(nmt),
                                              C.byref(sq), C.byref(nsq)), "mirp_get_windows")
        return {"windows": _copy_out(self.lib, w, records.WINDOW_DTYPE, nw.value), "wpeaks": _copy_out(self.lib, pk, records.PEAK_DTYPE, npk.value),
                "matures": _copy_out(self.lib, mt, records.MATURE_DTYPE, nmt.value), "seq": _copy_out(self.lib, sq, np.uint8, nsq.value)}

    def get_window_readtable(self):
        """int32 [n_windows, width, 3]: {length of the most abundant read, its depth, total depth} per start position ws + x of the window's strand."""
        t, w, n = C.c_void_p(), C.c_int32(), C.c_int64()
        self._check(self.lib.mirp_get_window_readtable(self.h, C.byref(t), C.byref(w), C.byref(n)), "mirp_get_window_readtable")
        return _copy_out(self.lib, t, np.int32, n.value * w.value * 3).reshape(n.value, w.value, 3)

    FOLD_MODELS = {"vienna-2.1.2": 0, "vienna-1.8.5": 1}

    def set_fold_model(self, model):
        """Which RNALfold the fold entry points reproduce: "vienna-2.1.2" (Turner-2004, dangles 2; default) or "vienna-1.8.5"
        (Turner-1999, dangles 1: the Linux binary the reference bundles)."""
        if model not in self.FOLD_MODELS:
            raise MirpError("unknown fold model %r (expected one of %s)" % (model, ", ".join(sorted(self.FOLD_MODELS))))
        self._check(self.lib.mirp_set_fold_model(self.h, self.FOLD_MODELS[model]), "mirp_set_fold_model")

    def set_contig_shard(self, preceded_by_coverage_elsewhere):
        """Contig sharding: see mirp_set_contig_shard in include/mirprefer.h."""
        self._check(self.lib.mirp_set_contig_shard(self.h, 1 if preceded_by_coverage_elsewhere else 0), "mirp_set_contig_shard")

    def fold(self, span, max_lines=96):
        self._check(self.lib.mirp_fold(self.h, int(span), int(max_lines)), "mirp_fold")

    def last_fold_fallbacks(self):
        return int(self.lib.mirp_last_fold_fallbacks(self.h))

    def last_fold_overflow(self):
        return int(self.lib.mirp_last_fold_overflow(self.h))

    def excl_scan(self, values):
        """Exclusive prefix sums of an int32 array on the device (mirp_excl_scan_i32, the scan of the candidate stage's compactions) -> int64 [n + 1]."""
        v = np.ascontiguousarray(values, dtype=np.int32)
        out = np.zeros(len(v) + 1, dtype=np.int64)
        fn = self.lib.mirp_excl_scan_i32
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
        self._check(fn(self.h, v.ctypes.data if len(v) else None, len(v), out.ctypes.data), "mirp_excl_scan_i32")
        return out

    def _sort_hook(self, name, values, dtype, *widths):
        v = np.ascontiguousarray(values, dtype=dtype)
        out = np.empty_like(v)
        fn = getattr(self.lib, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64] + [C.c_int32] * len(widths) + [C.c_void_p]
        self._check(fn(self.h, v.ctypes.data if len(v) else None, len(v), *[int(w) for w in widths], out.ctypes.data if len(v) else None), name)
        return out

    def sort_alns(self, alns, posbits, tidbits):
        """The stable device sort of MirpAln records by tid << posbits | pos (mirp_sort_alns, the sort of the ingest) -> the sorted copy.  Like the two
        below it orders by whole 8-bit digits: the key bits [base, base + 8 * ceil(bits / 8)).  For tests."""
        from .synth import ALN_DTYPE
        return self._sort_hook("mirp_sort_alns", alns, ALN_DTYPE, posbits, tidbits)

    def sort_records(self, recs, bits):
        """The stable device sort of SORT_REC_DTYPE records by the low bits of `key` (mirp_sort_records, the sort of the read collapse) -> the sorted copy."""
        return self._sort_hook("mirp_sort_records", recs, SORT_REC_DTYPE, bits)

    def sort_u64(self, values, base, bits):
        """The stable device sort of uint64 values by the bits from `base` up (mirp_sort_u64, the sort of the align index and the key passes) -> the
        sorted copy."""
        return self._sort_hook("mirp_sort_u64", values, np.uint64, base, bits)

    def libqc_reads(self, data, name, adapter="", error_permille=100, overlap=None, sample=LIBQC_SAMPLE):
        """Profile of one raw FASTQ / FASTA text (bytes, already decompressed) (mirp_libqc_reads): the 3' adapter found from the
        first `sample` reads and three tables over all reads; name is what messages call the file.  adapter = "" uses the found adapter for the
        insert table, otherwise the given one; overlap None = the trim's default.  -> {adapter, status ("none" / "ok" / "unsure"), seed,
        seed_count, min_count, left_steps, left_stop ("purity" / "support" / "cap"), reads, sampled, with_adapter, dimers, raw_len [1025],
        cycles [1024, 6] = A C G T other qsum, insert [1025, 6] = A C G T other total, seconds}; seconds = {upload, split, records, k-mers +
        adapter, trim, tables}."""
        o = LibqcOpts()
        ad = adapter.encode() if isinstance(adapter, str) else bytes(adapter)
        o.adapter = ad
        o.adapter_len, o.error_permille, o.min_overlap, o.sample = len(ad), int(error_permille), 0 if overlap is None else int(overlap), int(sample)
        f = LibqcFound()
        st = (C.c_int64 * 4)()
        sec = (C.c_double * 6)()
        raw_len = np.zeros(1025, np.int64)
        cycles = np.zeros((1024, 6), np.int64)
        insert = np.zeros((1025, 6), np.int64)
        i64p = C.POINTER(C.c_int64)
        self._check(self.lib.mirp_libqc_reads(self.h, data, len(data), os.fsencode(name), C.byref(o), C.byref(f), st, raw_len.ctypes.data_as(i64p),
                                              cycles.ctypes.data_as(i64p), insert.ctypes.data_as(i64p), sec), "mirp_libqc_reads")
        code = f.seed_code
        return dict(zip(LIBQC_STATS, list(st)), adapter=f.adapter[:f.adapter_len].decode(), status=LIBQC_STATUS[f.status],
                    seed="".join("ACGT"[(code >> (22 - 2 * i)) & 3] for i in range(12)), seed_count=int(f.seed_count), min_count=int(f.min_count),
                    left_steps=int(f.left_steps), left_stop=LIBQC_STOPS[f.left_stop], raw_len=raw_len, cycles=cycles, insert=insert, seconds=list(sec))

    def libqc_last_table(self):
        """The 4^12 k-mer counters (uint32) of the last libqc_reads (mirp_libqc_last_table); None after a refused call."""
        out = np.empty(1 << 24, np.uint32)
        return out if self.lib.mirp_libqc_last_table(self.h, out.ctypes.data) == 0 else None

    def set_text_piece(self, nbytes):
        """Bytes of text that leave the device in one piece in target_scan, mimic_scan, align_reads and trim_reads (mirp_set_text_piece); 0 = the
        default, 1 GiB.  Lowered only to test the piece path; no output depends on it."""
        fn = self.lib.mirp_set_text_piece
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int64]
        self._check(fn(self.h, int(nbytes)), "mirp_set_text_piece")

    def text_pieces_last(self):
        """Non-empty pieces of text the last target_scan, mimic_scan, align_reads or trim_reads handed to its output (mirp_text_pieces_last)."""
        fn = self.lib.mirp_text_pieces_last
        fn.restype = C.c_int64
        fn.argtypes = [C.c_void_p]
        return int(fn(self.h))

    def limit_windows(self, n_keep):
        """Keeps the first n_keep windows of the last candidate() for the following stages (mirp_limit_windows)."""
        self._check(self.lib.mirp_limit_windows(self.h, int(n_keep)), "mirp_limit_windows")
        self._n_windows = int(n_keep)

    def exchange_bytes(self, blocks):
        """All-to-all of byte strings on the context's communicator: blocks[q] goes to rank q; returns the list of blocks received, by source rank."""
        W = len(blocks)
        cnt = np.array([len(b) for b in blocks], dtype=np.int64)
        blob = b"".join(blocks)
        recv, rcnt = C.c_void_p(), np.zeros(W, dtype=np.int64)
        self._check(self.lib.mirp_exchange_bytes(self.h, blob if blob else None, cnt.ctypes.data, C.byref(recv), rcnt.ctypes.data), "mirp_exchange_bytes")
        tot = int(rcnt.sum())
        raw = C.string_at(recv.value, tot) if tot else b""
        self.lib.mirp_free(recv)
        out, o = [], 0
        for r in range(W):
            out.append(raw[o:o + int(rcnt[r])]); o += int(rcnt[r])
        return out

    def set_fold_split_path(self, mode):
        """0: multiloop splits over split candidates (default), 1: the dense split loop for every window (same tables either way)."""
        self._check(self.lib.mirp_set_fold_split_path(self.h, int(mode)), "mirp_set_fold_split_path")

    def set_fold_overlap(self, chunk_windows):
        """-1: automatic (default), 0: off (serial path), N > 0: the epilogue of every chunk of N windows beside the fill of the next chunk."""
        self._check(self.lib.mirp_set_fold_overlap(self.h, int(chunk_windows)), "mirp_set_fold_overlap")

    def set_fold_overlap_tailfree(self, mode):
        """-1: automatic (default: on), 1: the fills of neighbouring chunks on two streams, no idle CUs at a chunk boundary, dense hand-offs folded
        behind the last epilogue, 0: fills in order on one stream with a dense pass per chunk.  Same results either way."""
        self._check(self.lib.mirp_set_fold_overlap_tailfree(self.h, int(mode)), "mirp_set_fold_overlap_tailfree")

    def set_fold_capacity(self, windows):
        """Windows whose slabs the fold holds on the device at once (0 = the default, 8 GiB of slabs): lowered only to test the sub-batch path."""
        self._check(self.lib.mirp_set_fold_capacity(self.h, int(windows)), "mirp_set_fold_capacity")

    def last_fold_overlap_chunks(self):
        """Chunks the last fold ran in; 0: the serial path."""
        return int(self.lib.mirp_last_fold_overlap_chunks(self.h))

    def last_fold_dense(self):
        return int(self.lib.mirp_last_fold_dense(self.h))

    def set_fold_dedup(self, on):
        """True (default): fold() folds each distinct window sequence once and copies the result to its duplicates; False: every window is folded.
        Same results and counters either way."""
        self._check(self.lib.mirp_set_fold_dedup(self.h, 1 if on else 0), "mirp_set_fold_dedup")

    def set_fold_dedup_hash_bits(self, bits):
        """For tests: low bits of the dedup hash that count (0 = all 64); with a few bits different windows collide everywhere."""
        self._check(self.lib.mirp_set_fold_dedup_hash_bits(self.h, int(bits)), "mirp_set_fold_dedup_hash_bits")

    def last_fold_duplicates(self):
        """Windows the last fold() skipped as duplicates of an earlier window."""
        return int(self.lib.mirp_last_fold_duplicates(self.h))

    def get_fold_duplicates(self):
        """int32 [n_windows]: the lowest earlier window with the same bytes for every window the last fold() skipped, -1 for the others."""
        d, n = C.c_void_p(), C.c_int64()
        self._check(self.lib.mirp_get_fold_duplicates(self.h, C.byref(d), C.byref(n)), "mirp_get_fold_duplicates")
        return _copy_out(self.lib, d, np.int32, n.value)

    def set_coverage_path(self, mode):
        """-1: by record density (default), 0: atomic scatter, 1: fused scan where the input allows it."""
        self._check(self.lib.mirp_set_coverage_path(self.h, int(mode)), "mirp_set_coverage_path")

    def last_coverage_fused(self):
        """True when the last coverage pass built its tiles from the sorted records in LDS (dense inputs), False for the atomic scatter path."""
        return bool(self.lib.mirp_last_coverage_fused(self.h))

    def fold_summary(self):
        vp = C.c_void_p
        nl, mfe, st, n = vp(), vp(), vp(), C.c_int64()
        self._check(self.lib.mirp_get_fold_summary(self.h, C.byref(nl), C.byref(mfe), C.byref(st), C.byref(n)), "mirp_get_fold_summary")
        return {"n_lines": _copy_out(self.lib, nl, np.int32, n.value), "mfe": _copy_out(self.lib, mfe, np.int32, n.value),
                "status": _copy_out(self.lib, st, np.int32, n.value)}

    def fold_status(self):
        return self.fold_summary()["status"]

    def write_fold_text(self, fasta_path, out_path, wait=True):
        """RNALfold-format text of the resident fold output.  wait=False: returns once the output is off the device; formatting and writing go on
        in the library's worker threads (wait_text joins them)."""
        fn = self.lib.mirp_write_fold_text if wait else self.lib.mirp_write_fold_text_async
        self._check(fn(self.h, str(fasta_path).encode(), str(out_path).encode()), "mirp_write_fold_text")

    def wait_text(self):
        self._check(self.lib.mirp_wait_text(self.h), "mirp_wait_text")

    def write_depth_text(self, path, contig_names):
        """bam.depth.cut<CUT> of the last candidate() (MP:937-949), written by the library's worker threads."""
        blob = b"".join(n.encode() + b"\0" for n in contig_names)
        self._check(self.lib.mirp_write_depth_text(self.h, str(path).encode(), blob, len(contig_names)), "mirp_write_depth_text")

    def write_window_fasta(self, path, contig_names):
        """<prefix>.rnalfold.in_<i>.fa of the last candidate(): header + sequence of every window (MP:1124-1142)."""
        blob = b"".join(n.encode() + b"\0" for n in contig_names)
        self._check(self.lib.mirp_write_window_fasta(self.h, str(path).encode(), blob, len(contig_names)), "mirp_write_window_fasta")

    def get_fold(self):
        vp = C.c_void_p
        lines, ss, nl, mfe, st = vp(), vp(), vp(), vp(), vp()
        stride, ml = C.c_int32(), C.c_int32()
        self._check(self.lib.mirp_get_fold(self.h, C.byref(lines), C.byref(ss), C.byref(stride), C.byref(ml), C.byref(nl), C.byref(mfe), C.byref(st)),
                    "mirp_get_fold")
        n, stride, ml = self._n_windows, stride.value, ml.value
        raw = {"lines": _copy_out(self.lib, lines, FOLD_LINE_DTYPE, n * ml).reshape(n, ml),
               "ss": _copy_out(self.lib, ss, np.uint8, n * ml * stride).reshape(n, ml, stride), "stride": stride, "max_lines": ml,
               "n_lines": _copy_out(self.lib, nl, np.int32, n), "mfe": _copy_out(self.lib, mfe, np.int32, n),
               "status": _copy_out(self.lib, st, np.int32, n)}
        raw["overflow"] = self.fold_overflow()
        return raw

    def fold_overflow(self):
        """Windows of the last fold() that needed more structure lines than the main buffers hold (mirp_get_fold_overflow):
        {window index: (lines[max_lines2], ss[max_lines2, stride])}; use fold_window_lines() to read any window's lines."""
        vp = C.c_void_p
        wl, lines, ss, nl = vp(), vp(), vp(), vp()
        n, stride, ml = C.c_int64(), C.c_int32(), C.c_int32()
        self._check(self.lib.mirp_get_fold_overflow(self.h, C.byref(wl), C.byref(n), C.byref(lines), C.byref(ss), C.byref(stride), C.byref(ml), C.byref(nl)),
                    "mirp_get_fold_overflow")
        n, stride, ml = n.value, stride.value, ml.value
        wins = _copy_out(self.lib, wl, np.int32, n)
        a_l = _copy_out(self.lib, lines, FOLD_LINE_DTYPE, n * ml).reshape(n, ml)
        a_s = _copy_out(self.lib, ss, np.uint8, n * ml * stride).reshape(n, ml, stride)
        _copy_out(self.lib, nl, np.int32, n)
        return {int(w): (a_l[k], a_s[k]) for k, w in enumerate(wins)}

    def predict_raw(self, n_samples, min_mature_len, max_mature_len, allow_3nt, allow_no_star, minlen=55):
        """mirp_predict with the result left in flat arrays: {"result": MIRNA_DTYPE[n], "text": uint8[n, stride] structure rows, "n_passed", "status"};
        nothing is turned into Python objects per locus (write_result_reports takes the arrays as they are)."""
        from . import records
        pp = (C.c_int32 * 6)(int(n_samples), int(min_mature_len), int(max_mature_len), 1 if allow_3nt else 0, 1 if allow_no_star else 0, int(minlen))
        vp = C.c_void_p
        res, text, npass, stat = vp(), vp(), vp(), vp()
        nres, nw, stride = C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.mirp_predict(self.h, pp, C.byref(res), C.byref(nres), C.byref(text), C.byref(stride), C.byref(npass), C.byref(stat), C.byref(nw)),
                    "mirp_predict")
        r = _copy_out(self.lib, res, records.MIRNA_DTYPE, nres.value)
        t = _copy_out(self.lib, text, np.uint8, nres.value * stride.value).reshape(nres.value, max(stride.value, 1))
        return {"result": r, "text": t, "n_passed": _copy_out(self.lib, npass, np.int32, nw.value), "status": _copy_out(self.lib, stat, np.int32, nw.value)}

    def fold_predict_report_stream(self, span, params, n_chunks, contig_names, contig_arrays, alns, sample_names, mirbase_form, outdir, prefix, max_lines=96):
        """mirp_fold_predict_report_stream: fold + filter of the resident windows in chunks, a chunk's read-mapping files written by a host thread while the
        device folds the next chunk, the seven report files at the end.  params = (n_samples, min_mature_len, max_mature_len, allow_3nt, allow_no_star,
        minlen).  -> (number of miRNA loci, chunks used, device seconds {fold, predict})."""
        pp = (C.c_int32 * 6)(*[int(x) for x in params])
        alns = np.ascontiguousarray(alns)
        keep = [np.ascontiguousarray(a, dtype=np.uint8) if a is not None and len(a) else None for a in contig_arrays]
        ptrs = (C.c_void_p * max(len(keep), 1))(*[a.ctypes.data if a is not None else None for a in keep])
        lens = np.array([len(a) if a is not None else 0 for a in keep] or [0], dtype=np.int64)
        blob = lambda xs: b"".join(x.encode() + b"\0" for x in xs)
        nl, nc, ms = C.c_int64(), C.c_int32(), (C.c_double * 2)()
        fn = self.lib.mirp_fold_predict_report_stream
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_int32,
                       C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
        self._check(fn(self.h, int(span), int(max_lines), pp, int(n_chunks), blob(contig_names), len(contig_names), ptrs, lens.ctypes.data,
                       alns.ctypes.data if len(alns) else None, len(alns), blob(sample_names), len(sample_names), blob(mirbase_form), str(outdir).encode(), str(prefix).encode(),
                       C.byref(nl), C.byref(nc), ms), "mirp_fold_predict_report_stream")
        return int(nl.value), int(nc.value), {"fold_s": ms[0] / 1e3, "predict_s": ms[1] / 1e3}

    def select_windows(self, first, count):
        """mirp_select_windows: the fold and the filter run on windows [first, first + count) until changed; count < 0 = the whole list again."""
        self.lib.mirp_select_windows.argtypes = [C.c_void_p, C.c_int64, C.c_int64]
        self.lib.mirp_select_windows.restype = C.c_int
        self._check(self.lib.mirp_select_windows(self.h, int(first), int(count)), "mirp_select_windows")

    def predict(self, n_samples, min_mature_len, max_mature_len, allow_3nt, allow_no_star, minlen=55):
        from . import records
        pp = (C.c_int32 * 6)(int(n_samples), int(min_mature_len), int(max_mature_len), 1 if allow_3nt else 0, 1 if allow_no_star else 0, int(minlen))
        vp = C.c_void_p
        res, text, npass, stat = vp(), vp(), vp(), vp()
        nres, nw, stride = C.c_int64(), C.c_int64(), C.c_int32()
        self._check(self.lib.mirp_predict(self.h, pp, C.byref(res), C.byref(nres), C.byref(text), C.byref(stride), C.byref(npass), C.byref(stat), C.byref(nw)),
                    "mirp_predict")
        r = _copy_out(self.lib, res, records.MIRNA_DTYPE, nres.value)
        t = _copy_out(self.lib, text, np.uint8, nres.value * stride.value).reshape(nres.value, stride.value)
        tb, st = t.tobytes(), int(stride.value)
        ss = [tb[o:o + l].decode("ascii") for o, l in zip(range(0, len(tb), st), r["ss_len"].tolist())] if len(r) else []
        return {"result": r, "ss": ss, "n_passed": _copy_out(self.lib, npass, np.int32, nw.value), "status": _copy_out(self.lib, stat, np.int32, nw.value)}

    def predict_reasons(self, n_samples, min_mature_len, max_mature_len, allow_3nt, allow_no_star, minlen=55):
        """-d mode: int32 records [n, stride] of mirp_predict_reasons (layout in include/mirprefer.h), sorted by (window, mature, structure);
        the per-window records (mature index -1) come first within their window."""
        pp = (C.c_int32 * 6)(int(n_samples), int(min_mature_len), int(max_mature_len), 1 if allow_3nt else 0, 1 if allow_no_star else 0, int(minlen))
        rec, n, stride = C.c_void_p(), C.c_int64(), C.c_int32()
        self._check(self.lib.mirp_predict_reasons(self.h, pp, C.byref(rec), C.byref(n), C.byref(stride)), "mirp_predict_reasons")
        a = _copy_out(self.lib, rec, np.int32, n.value * stride.value).reshape(n.value, stride.value)
        if len(a):
            a = a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
        return a

    def last_fold_kernel_ms(self):
        """(fill ms, epilogue ms) of the last fold(), HIP events; with fold overlap: (first fill's start to last fill's end, the exposed rest)."""
        ms = (C.c_double * 2)()
        self.lib.mirp_last_fold_kernel_ms(self.h, ms)
        return ms[0], ms[1]

    def microbench(self):
        """Measured roofs of the fill kernel on this GPU (mirp_microbench): wave-instructions per second."""
        out = (C.c_double * 4)()
        self._check(self.lib.mirp_microbench(self.h, out), "mirp_microbench")
        return {"ds_read_b32_per_s": out[0], "ds_read_u16_per_s": out[1], "valu_pk16_per_s": out[2], "valu_u32_per_s": out[3]}

    def last_timings(self):
        ms = (C.c_double * 4)()
        self.lib.mirp_last_timings(self.h, ms)
        return {"coverage_ms": ms[0], "candidate_rest_ms": ms[1], "fold_ms": ms[2], "predict_ms": ms[3]}
