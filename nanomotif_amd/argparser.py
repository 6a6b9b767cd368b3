"""Command line of the MI355X build: the ``motif_discovery`` sub-command with the reference's arguments
(nanomotif/argparser.py:13-136), plus ``--device`` for the GPU to use, the project's own ``motif_sites`` / ``motif_coverage`` /
``motif_compare`` / ``motif_strands`` / ``motif_profile`` / ``motif_tracks`` / ``motif_fractions`` / ``motif_pileup`` / ``motif_shift`` / ``motif_context`` / ``motif_gc`` / ``motif_overlap`` / ``motif_regions`` / ``motif_runs`` on a finished ``bin-motifs.tsv``, ``motif_kmers`` (which needs none), and the binnary sub-commands ``detect_contamination`` and
``include_contigs`` with the reference's flags (argparser.py:139-236).  MTase-linker is out of scope."""
import argparse

__version__ = "1.1.2+mi355x.r1"


def create_parser():
    formatter = lambda prog: argparse.HelpFormatter(prog, max_help_position=28)
    parser = argparse.ArgumentParser(prog="nanomotif", description="Motif identification (MI355X-native motif_discovery)",
                                     formatter_class=formatter)
    parser.add_argument("--version", action="version", version="%(prog)s {}".format(__version__))
    sub = parser.add_subparsers(help="-- Command descriptions --", dest="command", title="commands",
                                metavar="{motif_discovery, motif_sites, motif_coverage, motif_compare, motif_strands, motif_profile, motif_tracks, motif_fractions, motif_pileup, motif_shift, motif_context, motif_gc, motif_overlap, motif_regions, motif_runs, motif_kmers, detect_contamination, include_contigs, check_installation}")
    p = sub.add_parser("motif_discovery", help="Finds motifs directly on bin level in provided assembly", add_help=False)
    p.add_argument("assembly", type=str, help="path to the assembly file.")
    p.add_argument("pileup", type=str, help="path to the modkit pileup file.")
    gm = p.add_argument_group("contig bin arguments, use one of:")
    g = gm.add_mutually_exclusive_group(required=True)
    g.add_argument("-c", "--contig_bin", type=str, help="TSV file specifying which bin contigs belong.")
    g.add_argument("-f", "--files", nargs="+", help="List of bin FASTA files with contig names as headers.")
    g.add_argument("-d", "--directory", help="Directory containing bin FASTA files with contig names as headers.")
    gm.add_argument("--extension", type=str, default=".fasta",
                    help="File extension of the bin FASTA files if using -d (DIRECTORY) argument. Default is '.fasta'.")
    o = p.add_argument_group("Options")
    o.add_argument("--out", type=str, help="path to the output folder", default="nanomotif")
    o.add_argument("--methylation_threshold_low", type=float, default=0.30,
                   help="A position is considered non-methylated if fraction of methylation is below this threshold. Default: %(default)s")
    o.add_argument("--methylation_threshold_high", type=float, default=0.70,
                   help="A position is considered methylated if fraction of methylated reads is above this threshold. Default: %(default)s")
    o.add_argument("--search_frame_size", type=int, default=40,
                   help="length of the sequnces sampled around confident methylation sites. Default: %(default)s")
    o.add_argument("--minimum_kl_divergence", type=float, default=0.05,
                   help="Minimum KL-divergence for a position to considered for expansion in  motif search. Default: %(default)s")
    o.add_argument("--min_motif_score", type=float, default=1.5,
                   help="Minimum score for a motif to be kept after identification. Default: %(default)s")
    o.add_argument("--threshold_valid_coverage", type=int, default=5,
                   help="Minimum valid base coverage (Nvalid_cov) for a position to be considered. Default: %(default)s")
    o.add_argument("--min_motifs_bin", type=int, default=50,
                   help="Minimum number of motif observations in a bin. Default: %(default)s")
    o.add_argument("--device", type=int, default=None, help="GPU to use (default: LOCAL_RANK or 0).")
    o.add_argument("--shard", choices=["auto", "bins", "contigs"], default="auto",
                   help="Multi-GPU runs: give every GPU whole bins (independent searches, no collective) or shard the "
                        "contigs of every bin over the GPUs (count tables all-reduced per round). Default: bins when "
                        "they balance within 15%%, else contigs.")
    gen = p.add_argument_group("general arguments")
    gen.add_argument("-t", "--threads", type=int, default=1, help="Accepted for compatibility; the GPU engine does not use worker processes.")
    gen.add_argument("-v", "--verbose", action="store_true", help="Increase output verbosity. (set logger to debug level)")
    gen.add_argument("--seed", type=int, default=1, help="Seed for random number generator. Default: %(default)s")
    gen.add_argument("-h", "--help", action="help", help="show this help message and exit")
    add_motif_sites_parser(sub)
    add_motif_coverage_parser(sub)
    add_motif_compare_parser(sub)
    add_motif_strands_parser(sub)
    add_motif_profile_parser(sub)
    add_motif_tracks_parser(sub)
    add_motif_fractions_parser(sub)
    add_motif_pileup_parser(sub)
    add_motif_shift_parser(sub)
    add_motif_context_parser(sub)
    add_motif_gc_parser(sub)
    add_motif_overlap_parser(sub)
    add_motif_regions_parser(sub)
    add_motif_runs_parser(sub)
    add_motif_kmers_parser(sub)
    add_binnary_parsers(sub)
    sub.add_parser("check_installation", help="Run motif_discovery on a small synthetic data set", add_help=True)
    return parser


# ------------------------------------------------------------------------------------------------ what the export commands share
def _selection(constant):
    """An argparse ``type``: a comma-separated selection of the names in ``engine.<constant>``, returned in that tuple's order.  The
    engine is imported when the first value is parsed, not when the parser is made."""
    def parse(text):
        from . import engine
        names = getattr(engine, constant)
        asked = [s.strip() for s in text.split(",") if s.strip()]
        if not asked or any(s not in names for s in asked):
            raise argparse.ArgumentTypeError(f"a comma-separated selection of {', '.join(names)} is expected, got {text!r}")
        return tuple(s for s in names if s in asked)
    return parse


def _checked(module, function, keep_text=False):
    """An argparse ``type`` from ``nanomotif_amd.<module>.<function>``: its ValueError becomes the parser's error.  The module is
    imported when the first value is parsed, not when the parser is made.  ``keep_text``: check only, the option keeps the text."""
    def parse(text):
        from importlib import import_module
        try:
            value = getattr(import_module("." + module, __package__), function)(text)
        except ValueError as e:
            raise argparse.ArgumentTypeError(str(e)) from None
        return text if keep_text else value
    return parse


def _open_export(sub, name, help, bin_motifs=None, many=True, pileups=(("pileup", "path to the modkit pileup file."),)):
    """Opens the subparser of an export command: assembly, pileup(s) and bins spelled as for motif_discovery (the pileup is ingested the
    same way), then "Options" with ``--bin_motifs`` (``bin_motifs``: its help; ``many``: several paths or one; None: the command places
    the option itself) and ``--out``.  Returns (parser, its "Options" group): the command adds its own options, then ``_close_export``."""
    p = sub.add_parser(name, help=help, add_help=False)
    p.add_argument("assembly", type=str, help="path to the assembly file.")
    for dest, text in pileups:
        p.add_argument(dest, type=str, help=text)
    gm = p.add_argument_group("contig bin arguments, use one of:")
    g = gm.add_mutually_exclusive_group(required=True)
    g.add_argument("-c", "--contig_bin", type=str, help="TSV file specifying which bin contigs belong.")
    g.add_argument("-f", "--files", nargs="+", help="List of bin FASTA files with contig names as headers.")
    g.add_argument("-d", "--directory", help="Directory containing bin FASTA files with contig names as headers.")
    gm.add_argument("--extension", type=str, default=".fasta",
                    help="File extension of the bin FASTA files if using -d (DIRECTORY) argument. Default is '.fasta'.")
    o = p.add_argument_group("Options")
    if bin_motifs is not None:
        o.add_argument("--bin_motifs", type=str, required=True, help=bin_motifs, **({"nargs": "+"} if many else {}))
    o.add_argument("--out", type=str, help="path to the output folder", default="nanomotif")
    return p, o


def _close_export(p, o, filters="calls", more=()):
    """Closes the subparser of an export command: the filter block — "calls": the three call thresholds; "reads": the two read filters of
    the commands that read the pileup as READ STATISTICS; "reads and zones": those and the two thresholds as histogram zones — then
    ``more`` ((flag, keywords) of options the command keeps behind the block), ``--device`` and the general arguments."""
    if filters != "calls":
        o.add_argument("--min_valid_read_coverage", type=int, default=5,
                       help="Minimum valid base coverage (Nvalid_cov) for a pileup record to be read. Default: %(default)s")
        o.add_argument("--min_valid_cov_to_diff_fraction", type=float, default=0.8,
                       help="Minimum Nvalid_cov / (Nvalid_cov + Ndiff) for a pileup record to be read. Default: %(default)s")
    if filters != "reads":
        low, high = (("Upper edge of the unmethylated zone, snapped to a bin edge.", "Lower edge of the methylated zone, snapped to a bin edge.")
                     if filters == "reads and zones" else
                     ("A position is considered non-methylated if fraction of methylation is below this threshold.",
                      "A position is considered methylated if fraction of methylated reads is above this threshold."))
        o.add_argument("--methylation_threshold_low", type=float, default=0.30, help=low + " Default: %(default)s")
        o.add_argument("--methylation_threshold_high", type=float, default=0.70, help=high + " Default: %(default)s")
    if filters == "calls":
        o.add_argument("--threshold_valid_coverage", type=int, default=5,
                       help="Minimum valid base coverage (Nvalid_cov) for a position to be considered. Default: %(default)s")
    for flag, keywords in more:
        o.add_argument(flag, **keywords)
    o.add_argument("--device", type=int, default=None, help="GPU to use (default: LOCAL_RANK or 0).")
    gen = p.add_argument_group("general arguments")
    gen.add_argument("-t", "--threads", type=int, default=1, help="Threads of the file readers.")
    gen.add_argument("-v", "--verbose", action="store_true", help="Increase output verbosity. (set logger to debug level)")
    gen.add_argument("--seed", type=int, default=1, help=argparse.SUPPRESS)
    gen.add_argument("-h", "--help", action="help", help="show this help message and exit")


# ------------------------------------------------------------------------------------------------ the commands: what is their own
def add_motif_sites_parser(sub):
    """motif_sites: the per-site view of a bin-motifs.tsv (no counterpart on the reference's command line; the data are what
    motif_model_contig(save_motif_positions=True) returns, find_motifs_bin.py:1285-1331)."""
    p, o = _open_export(sub, "motif_sites", "Exports where the motifs of a bin-motifs.tsv occur and which occurrences are methylated",
                        "Path to the bin-motifs.tsv whose motifs are exported (motif_discovery's output)", many=False)
    o.add_argument("--states", type=_selection("SITE_STATES"), default=("mod", "nomod", "nocall"),
                   help="Comma-separated states of the occurrences to export: mod, nomod, nocall. Default: all three")
    _close_export(p, o)


def add_motif_coverage_parser(sub):
    """motif_coverage: how much of a bin's methylation the motifs of a bin-motifs.tsv explain (the reference only logs "% of sequences
    remaining" inside find_best_candidates, find_motifs_bin.py:801-823)."""
    p, o = _open_export(sub, "motif_coverage", "Reports how much of each bin's methylation the motifs of a bin-motifs.tsv explain",
                        "Path to the bin-motifs.tsv whose motifs are assessed (motif_discovery's output)", many=False)
    o.add_argument("--unexplained_sites", action="store_true",
                   help="Also write unexplained-sites.bed: the methylated positions no motif of their bin covers")
    _close_export(p, o)


def add_motif_compare_parser(sub):
    """motif_compare: per-motif methylation change between two pileups of one assembly (no counterpart on the reference's command line;
    nearest: two runs of motif_model_contig(save_motif_positions=True), find_motifs_bin.py:1285-1331, joined by hand).  Both pileups are
    ingested as motif_discovery ingests its one."""
    p, o = _open_export(sub, "motif_compare", "Compares the methylation of the motifs of bin-motifs.tsv files between two pileups of one assembly",
                        "Path(s) to the bin-motifs.tsv whose motifs are compared (typically motif_discovery's output on sample A and on sample B)",
                        pileups=(("pileup_a", "path to the modkit pileup file of sample A."),
                                 ("pileup_b", "path to the modkit pileup file of sample B (same assembly).")))
    o.add_argument("--switched_sites", action="store_true",
                   help="Also write switched-sites.bed: the occurrences whose state changed between the samples (see --transitions)")
    o.add_argument("--transitions", type=_selection("TRANSITIONS"), default=("mod>nomod", "nomod>mod"),
                   help="Comma-separated transitions A>B written to switched-sites.bed, each of mod, nomod, nocall on either side. "
                        "Default: mod>nomod,nomod>mod")
    _close_export(p, o)


def add_binnary_parsers(sub):
    """detect_contamination / include_contigs (argparser.py:139-236): flags, defaults and help of the reference."""
    shared = argparse.ArgumentParser(description="Contamination DNA Methylation Pattern", add_help=False)
    mandatory = shared.add_argument_group("Mandatory Arguments")
    mandatory.add_argument("--pileup", type=str, help="Path to pileup.bed", required=True)
    mandatory.add_argument("--assembly", type=str, help="Path to assembly file [fasta format required]", required=True)
    mandatory.add_argument("--bin_motifs", type=str, help="Path to bin-motifs.tsv file", required=True)
    mandatory.add_argument("--contig_bins", type=str, help="Path to bins.tsv file for contig bins", required=True)
    shared.add_argument("-t", "--threads", type=int, default=1, help="Number of threads to use for multiprocessing")
    shared.add_argument("--min_valid_read_coverage", type=int, default=3,
                        help="Minimum read coverage for calculating methylation [used with methylation_util executable]")
    shared.add_argument("--methylation_threshold", type=int, default=24,
                        help="Filtering criteria for trusting contig methylation. It is the product of mean_read_coverage and "
                             "N_motif_observation. Higher value means stricter criteria. [default: 24]")
    shared.add_argument("--num_consensus", type=int, default=4, help="Number of models that has to agree for classifying as contaminant")
    shared.add_argument("--force", action="store_true",
                        help="Force override of motifs-scored-read-methylation.tsv. If not set existing file will be used.")
    shared.add_argument("--write_bins", action="store_true",
                        help="If specified, new bins will be written to a bins folder. Requires --assembly_file to be specified.")
    shared.add_argument("--methylation_output_type", default="median", choices=["median", "weighted_mean"],
                        help="Specify whether to use the median of mean methylated motif positions or the weighted mean. [default: median]")
    mandatory.add_argument("--out", type=str, help="Path to output directory", required=True, default="nanomotif")
    shared.add_argument("--device", type=int, default=None, help="GPU to use (default: LOCAL_RANK or 0).")

    cont = sub.add_parser("detect_contamination", help="Detect contamination in bins", parents=[shared])
    cont.add_argument("--contamination_file", type=str,
                      help="Path to an existing contamination file if bins should be outputtet as a post-processing step")

    inc = sub.add_parser("include_contigs", help="Include contigs in bins", parents=[shared])
    inc.add_argument("--mean_model_confidence", type=float, default=0.8,
                     help="Mean probability between models for including contig. Contigs above this value will be included. [default: 0.8]")
    group = inc.add_mutually_exclusive_group(required=False)
    group.add_argument("--contamination_file", type=str, help="Path to an existing contamination file to include in the analysis")
    group.add_argument("--run_detect_contamination", action="store_true",
                       help="Indicate that the detect_contamination workflow should be run first")


def add_motif_strands_parser(sub):
    """motif_strands: the state of both strands of every motif site — full, hemi, unmethylated (no counterpart on the reference's command
    line, which pairs a motif with its complement by name only; modkit has pileup-hemi for CpG)."""
    p, o = _open_export(sub, "motif_strands", "Reports whether both strands of the motif sites of bin-motifs.tsv files are methylated",
                        "Path(s) to the bin-motifs.tsv whose motif sites are assessed (motif_discovery's output)")
    o.add_argument("--hemi_sites", action="store_true",
                   help="Also write hemi-sites.bed: the occurrences whose own base and partner base differ in state (see --pairs)")
    o.add_argument("--pairs", type=_selection("PAIRS"), default=("mod-nomod", "nomod-mod"),
                   help="Comma-separated pairs own-partner written to hemi-sites.bed, each of mod, nomod, nocall on either side. "
                        "Default: mod-nomod,nomod-mod")
    _close_export(p, o)


def add_motif_profile_parser(sub):
    """motif_profile: the methylation of every position around the sites of the motifs of bin-motifs.tsv files, both strands, every mod
    type of the pileup (no counterpart on the reference's command line)."""
    p, o = _open_export(sub, "motif_profile", "Reports the methylation at every offset around the motif sites of bin-motifs.tsv files",
                        "Path(s) to the bin-motifs.tsv whose motif sites are profiled (motif_discovery's output)")
    o.add_argument("--radius", type=_checked("motif_profile", "parse_radius"), default=10,
                   help="Offsets either side of the modified base that are profiled, 0..31. Default: %(default)s")
    o.add_argument("--targets", type=_checked("motif_profile", "parse_targets"), default=None,
                   help="Comma-separated mod types whose calls are read at every offset: a, m, 21839. Default: every mod type the pileup holds rows of")
    o.add_argument("--min_called", type=int, default=20,
                   help="Called sites a cell needs to be considered for the summary's best cell. Default: %(default)s")
    _close_export(p, o)


def add_motif_context_parser(sub):
    """motif_context: the letter at every offset around the sites of the motifs of bin-motifs.tsv files, counted apart by the state of the
    site: which position and letters separate the methylated sites from the rest (no counterpart on the reference's command line)."""
    p, o = _open_export(sub, "motif_context", "Reports the sequence context of the motif sites of bin-motifs.tsv files by methylation state",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--radius", type=_checked("motif_context", "parse_radius"), default=10,
                   help="Offsets either side of the modified base whose letters are counted, 0..31. Default: %(default)s")
    o.add_argument("--min_called", type=int, default=20,
                   help="Called sites a motif needs to be judged, and the dropped letters need for the underspecified flag. Default: %(default)s")
    o.add_argument("--min_gain", type=float, default=30.0,
                   help="Log-likelihood gain of the best offset's split by letter from which a motif is flagged underspecified. Default: %(default)s")
    _close_export(p, o)


def add_motif_gc_parser(sub):
    """motif_gc: the methylation of the motifs of bin-motifs.tsv files stratified by the GC content around their sites, beside the bin's
    background: is a motif methylated everywhere, or where the local GC is high (no counterpart on the reference's command line; its
    known-issues page advises to check high-GC 5mC noise by hand)."""
    p, o = _open_export(sub, "motif_gc", "Reports the methylation of the motifs of bin-motifs.tsv files by the GC content around their sites",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--half", type=_checked("motif_gc", "parse_half"), default=31,
                   help="Positions either side of the modified base in the GC window, 0..31 (the window is 2 HALF + 1 positions). Default: %(default)s")
    o.add_argument("--gc_bins", type=_checked("motif_gc", "parse_gc_bins"), default=8,
                   help="Buckets of local GC the sites are written in (at most one per count of G + C). Default: %(default)s")
    o.add_argument("--min_called", type=int, default=20, help="Called sites a motif needs to be judged. Default: %(default)s")
    o.add_argument("--min_z", type=float, default=5.0,
                   help="|trend_z_within| from which a motif can be flagged gc_dependent. Default: %(default)s")
    o.add_argument("--min_delta", type=float, default=0.2,
                   help="|frac_mod of the high-GC third - frac_mod of the low-GC third| from which a motif can be flagged gc_dependent. Default: %(default)s")
    _close_export(p, o)


def add_motif_overlap_parser(sub):
    """motif_overlap: the sites the motifs of one bin share, which motif is nested in which, and how methylated a motif is outside the
    motifs nested in it (the reference settles nesting by the motifs' spelling, postprocess.py)."""
    p, o = _open_export(sub, "motif_overlap", "Reports shared sites and nesting between the motifs of each bin of bin-motifs.tsv files",
                        "Path(s) to the bin-motifs.tsv whose motifs are compared (motif_discovery's output)")
    o.add_argument("--all_pairs", action="store_true", help="Also write the pairs of motifs that share no site")
    o.add_argument("--min_called", type=int, default=20, help="Called sites a motif, or a part of one, needs to be judged. Default: %(default)s")
    o.add_argument("--max_outside", type=float, default=0.3,
                   help="Fraction of methylation outside its children up to which a motif can be flagged carried_by_children. Default: %(default)s")
    o.add_argument("--min_frac", type=float, default=0.7,
                   help="Fraction of methylation from which a part of a motif counts as methylated (carried_by_children, submotif). Default: %(default)s")
    _close_export(p, o)


def add_motif_regions_parser(sub):
    """motif_regions: the methylation of the motifs of bin-motifs.tsv files inside the classes of a BED / GFF3 annotation — prophages,
    genes and what lies in front of them, repeat masks — beside the bin's background (no counterpart on the reference's command line;
    people intersect motif-sites.bed with bedtools and group by hand)."""
    p, o = _open_export(sub, "motif_regions", "Reports the methylation of the motifs of bin-motifs.tsv files inside the regions of an annotation",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--regions", type=str, required=True, metavar="FILE",
                   help="BED or GFF3 file of annotated regions, plain or .gz. The class of an interval is BED column 4 (without it: region) / GFF3 column 3")
    o.add_argument("--classes", type=_checked("regions", "parse_classes"), default=None,
                   help="Comma-separated classes to read, in this order (at most 8). Default: every class, in order of first appearance")
    o.add_argument("--upstream", type=_checked("regions", "parse_upstream"), default=0,
                   help="Adds the class upstream: this many bases in front of every stranded interval. Default: %(default)s (off)")
    o.add_argument("--min_called", type=int, default=20, help="Called sites a class and the rest need for a motif to be judged. Default: %(default)s")
    o.add_argument("--min_z", type=float, default=5.0, help="|z| from which a motif can be flagged depleted / enriched in a class. Default: %(default)s")
    o.add_argument("--min_delta", type=float, default=0.2,
                   help="|frac_mod in the class - frac_mod of the rest| from which a motif can be flagged depleted / enriched. Default: %(default)s")
    o.add_argument("--region_sites", action="store_true", help="Also write region-sites.bed: the selected sites with the classes they are inside")
    o.add_argument("--states", type=_selection("SITE_STATES"), default=("mod", "nomod", "nocall"),
                   help="Comma-separated states of the sites of region-sites.bed: mod, nomod, nocall. Default: all three")
    o.add_argument("--inside", type=_checked("motif_regions", "parse_inside"), default=None,
                   help="Comma-separated classes (and / or outside) whose sites go to region-sites.bed. Default: every class")
    o.add_argument("--intervals", action="store_true", help="Also write motif-regions-intervals.tsv: the six counts per interval and motif")
    _close_export(p, o)


def add_motif_runs_parser(sub):
    """motif_runs: runs of consecutive same-state sites of the motifs of bin-motifs.tsv files along the contigs — footprints of
    unmethylated sites, alternating states of a strand-biased caller — with the Wald-Wolfowitz runs test beside the bin's background (no
    counterpart on the reference's command line; people export motif-sites.bed and group consecutive rows by hand)."""
    p, o = _open_export(sub, "motif_runs", "Reports runs of consecutive same-state motif sites of bin-motifs.tsv files along the contigs",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--max_run", type=_checked("motif_runs", "parse_max_run"), default=16,
                   help="Run lengths counted apart, 2..64: the last bucket of motif-runs-hist.tsv holds the runs of MAX_RUN sites or more. Default: %(default)s")
    o.add_argument("--nocall_breaks", action="store_true",
                   help="A site without a call takes part and ends a run. Default: such a site is transparent, it neither extends nor breaks a run")
    o.add_argument("--min_called", type=int, default=20, help="Called sites a motif needs to be judged. Default: %(default)s")
    o.add_argument("--min_z", type=float, default=5.0,
                   help="|runs_z_within| from which a motif is flagged clustered (negative) or alternating (positive). Default: %(default)s")
    o.add_argument("--runs", action="store_true", help="Also write motif-runs.bed: one line per run of --states with at least --min_run sites")
    o.add_argument("--states", type=_checked("motif_runs", "parse_run_states"), default=("nomod",),
                   help="Comma-separated states of the runs of motif-runs.bed: mod, nomod, and with --nocall_breaks nocall. Default: nomod")
    o.add_argument("--min_run", type=_checked("motif_runs", "parse_min_run"), default=3,
                   help="Sites a run needs to be written to motif-runs.bed, at least 1. Default: %(default)s")
    _close_export(p, o)


def add_motif_kmers_parser(sub):
    """motif_kmers: the methylation of every k-mer context of every bin, without a motif as input: what the greedy search missed and what
    it over-generalised (no counterpart on the reference's command line; modkit and nanodisco users know the table as the k-mer table).
    --bin_motifs is optional, and placed behind --shape."""
    p, o = _open_export(sub, "motif_kmers", "Reports the methylation of every k-mer context around the A / C of every bin")
    o.add_argument("--shape", type=_checked("engine", "kmer_shape", keep_text=True), default="NNN*NNN",
                   help="The counted positions: N counted, . skipped, exactly one * for the modified base; at most 10 N within 31 positions of "
                        "the *, e.g. 'NNN*......NNN'. Default: %(default)s")
    o.add_argument("--bin_motifs", type=str, nargs="+", default=None,
                   help="Path(s) to bin-motifs.tsv (motif_discovery's output): adds the columns implied_by / compatible_with and the files "
                        "kmer-unexplained.tsv and kmer-overcalled.tsv")
    o.add_argument("--min_called", type=int, default=20, help="Called sites (n_mod + n_nomod) a k-mer needs to be written. Default: %(default)s")
    o.add_argument("--min_frac", type=float, default=0.7,
                   help="frac_mod from which a k-mer no motif accounts for is written to kmer-unexplained.tsv. Default: %(default)s")
    _close_export(p, o)


def add_motif_tracks_parser(sub):
    """motif_tracks: the methylation of the motifs of bin-motifs.tsv files per window along the contigs of their bins, and its breakpoints
    (no counterpart on the reference's command line)."""
    p, o = _open_export(sub, "motif_tracks", "Reports the methylation of the motifs of bin-motifs.tsv files along contigs, and its breakpoints",
                        "Path(s) to the bin-motifs.tsv whose motifs are followed along the contigs (motif_discovery's output)")
    o.add_argument("--window", type=_checked("motif_tracks", "parse_window"), default=4096,
                   help="Window size in bp, a multiple of 128 in [128, 2^30]. Default: %(default)s")
    o.add_argument("--min_gain", type=float, default=30.0,
                   help="Likelihood-ratio gain a split needs to be accepted as a breakpoint. Default: %(default)s")
    o.add_argument("--min_called", type=int, default=20, help="Called sites either side of a split needs. Default: %(default)s")
    o.add_argument("--max_segments", type=int, default=8, help="Segments a contig is split into at the most. Default: %(default)s")
    o.add_argument("--tracks", action="store_true", help="Also write motif-tracks.tsv: the six counts of every window that holds an occurrence")
    _close_export(p, o)


def add_motif_fractions_parser(sub):
    """motif_fractions: the histogram of the read fractions n_modified / n_valid_cov over the sites of the motifs of bin-motifs.tsv files (no
    counterpart on the reference's command line).  The pileup is read as READ STATISTICS (binnary's filters), not as thresholded calls."""
    p, o = _open_export(sub, "motif_fractions", "Reports the distribution of the read fractions at the motif sites of bin-motifs.tsv files",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--bins", type=_checked("motif_fractions", "parse_bins"), default=20, help="Histogram bins over [0, 1], 2..64. Default: %(default)s")
    _close_export(p, o, "reads and zones", more=(
        ("--min_sites", dict(type=int, default=20, help="Sites below which a row is flagged few_sites. Default: %(default)s")),
        ("--minor_share", dict(type=float, default=0.1,
                               help="Share of the sites the smaller mode of a bimodal motif needs, and a methylated / unmethylated motif may miss. "
                                    "Default: %(default)s"))))


def add_motif_pileup_parser(sub):
    """motif_pileup: the n_valid_cov and n_modified of the pileup record under every site of the motifs of bin-motifs.tsv files (no
    counterpart on the reference's command line; modkit motif bed + bedtools intersect yield the table).  The arguments of
    motif_fractions without the histogram options: the pileup read as READ STATISTICS."""
    p, o = _open_export(sub, "motif_pileup", "Reports the read counts under every motif site of bin-motifs.tsv files",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)")
    o.add_argument("--all_occurrences", action="store_true",
                   help="Also write the occurrences whose modified base carries no kept pileup record (0, 0 and an empty percentage)")
    _close_export(p, o, "reads")


def add_motif_shift_parser(sub):
    """motif_shift: the per-site change of the read fraction n_modified / n_valid_cov between two pileups of one assembly at the sites of the
    motifs of bin-motifs.tsv files (no counterpart on the reference's command line; `modkit dmr pair` with a motif BED and a join yield the
    table).  Both pileups are read as READ STATISTICS, as motif_fractions reads its one."""
    p, o = _open_export(sub, "motif_shift", "Reports how the read fractions at the motif sites of bin-motifs.tsv files change between two pileups",
                        "Path(s) to the bin-motifs.tsv whose motif sites are read (motif_discovery's output)",
                        pileups=(("pileup_a", "path to the modkit pileup file of sample A."),
                                 ("pileup_b", "path to the modkit pileup file of sample B (same assembly).")))
    o.add_argument("--bins", type=_checked("motif_shift", "parse_bins"), default=10, help="Bins per axis of the joint histogram, 2..16. Default: %(default)s")
    o.add_argument("--min_delta", type=_checked("motif_shift", "parse_min_delta"), default=250,
                   help="Difference of the two read fractions from which a site counts as shifted: 0..1 with at most three decimals. Default: 0.25")
    o.add_argument("--shifted_sites", action="store_true", help="Also write shifted-sites.bed: the shifted sites (see --directions)")
    o.add_argument("--directions", type=_selection("SHIFT_SELECT"), default=("up", "down"),
                   help="Comma-separated directions A to B written to shifted-sites.bed: up, down. Default: up,down")
    _close_export(p, o, "reads and zones", more=(
        ("--min_sites", dict(type=int, default=20, help="Paired sites below which a row is flagged few_sites. Default: %(default)s")),
        ("--min_share", dict(type=float, default=0.5, help="Share of the paired sites that must be shifted in one direction for gained / lost. "
                                                           "Default: %(default)s")),
        ("--minor_share", dict(type=float, default=0.1, help="Share of the paired sites shifted in each direction from which a motif is mixed. "
                                                             "Default: %(default)s"))))
