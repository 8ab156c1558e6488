"""The options of the net-free search in one record: what gtp, match and selfplay take on their command lines
and NativeMCTS as keywords, declared once, checked once, and turned into the keywords of the next layer down.

    PlayoutOptions.add_arguments(parser)        the flags, one help text each
    PlayoutOptions.from_args(parser, args)      the record of a parsed command line; parser.error on a refused combination
    PlayoutOptions.from_keywords(kwargs)        the record of NativeMCTS's keywords; TypeError / ValueError
    .search_keywords()                          the keywords of NativeMCTS / NativeGTP: only the options that are set
    .evaluator_keywords()                       the keywords of rollout.PlayoutEvaluator
    .name_suffix()                              what match calls such an engine: -mc64-pat-amaf1-rave4-lgr (-lgr2 with pairs,
                                                -mast with move values, -nast with move contexts)

Nothing here imports torch or rollout: a front end parses its command line before it loads either.
"""
import dataclasses

FLAGS = {  # field -> (flag, what argparse needs, help)
    "playout_value": ("--playout-value", dict(type=int, default=0, metavar="N"),
                      "N > 0: no value net -- a leaf's value is the share of N random playouts its side to move wins"),
    "playout_patterns": ("--playout-patterns", dict(default=None, metavar="FILE"),
                         "with --playout-value: draw the playouts' moves by the 3x3 pattern weights of this table "
                         "(python -m bokego_amd.patterns fit)"),
    "playout_tactics": ("--playout-tactics", dict(default=None, metavar="FILE"),
                        "with --playout-value: multiply the playouts' weights by the tactical weights of this table "
                        "(python -m bokego_amd.tactics fit)"),
    "playout_prior": ("--playout-prior", dict(type=float, default=0.0, metavar="LAMBDA"),
                      "with --playout-value: that share (0..1) of the priors comes from the playouts' AMAF counts; with 1 "
                      "no policy net is loaded"),
    "playout_rave": ("--playout-rave", dict(type=float, nargs="?", const=4.0, default=0.0, metavar="K"),
                     "with --playout-value: RAVE -- the playouts' two-sided AMAF counts are backed up into per-node tables and "
                     "blended into the selection with the equivalence parameter K (visits; 4 when no value is given: the one "
                     "of 4, 16 and 64 that won its 100-game match, DESIGN 20)"),
    "playout_criticality": ("--playout-criticality", dict(type=float, default=0.0, metavar="GAMMA"),
                            "with --playout-prior: add GAMMA times Coulom's criticality of each point, from the final boards "
                            "of the same playouts, to the AMAF win rates the prior is made of (untuned; default 0: off, "
                            "DESIGN 21)"),
    "playout_pattern_prior": ("--playout-pattern-prior", dict(type=float, default=0.0, metavar="MU"),
                              "with --playout-prior: add MU times the log of each point's move weight -- the playouts' pattern "
                              "and tactical tables, or --prior-patterns / --prior-tactics -- to the prior's logits (untuned; "
                              "default 0: off, DESIGN 22)"),
    "prior_patterns": ("--prior-patterns", dict(default=None, metavar="FILE"),
                       "with --playout-pattern-prior: the pattern table of that term (default: --playout-patterns)"),
    "prior_tactics": ("--prior-tactics", dict(default=None, metavar="FILE"),
                      "with --playout-pattern-prior: the tactics table of that term (default: --playout-tactics)"),
    "playout_replies": ("--playout-replies", dict(action="store_true"),
                        "with --playout-value: the playouts of a search learn a last-good-reply table from each other and play "
                        "its replies where they are playable (untuned; default off, DESIGN 24)"),
    "playout_reply_pairs": ("--playout-reply-pairs", dict(action="store_true"),
                            "with --playout-value: as --playout-replies with replies keyed by the last two moves as well, the "
                            "single-move table being the fallback (LGRF-2; untuned; default off, DESIGN 26)"),
    "playout_move_contexts": ("--playout-move-contexts", dict(type=float, nargs="?", const=0.25, default=0.0, metavar="TAU"),
                              "with --playout-value: NAST -- as --playout-move-values with a win rate per colour, previous move "
                              "and point as well, averaged with the plain one once it has 8 plays and falling back to it before "
                              "(TAU 0.25 when no value is given: plausible and untuned; not with --playout-move-values; default "
                              "0: off, DESIGN 32)"),
    "playout_move_values": ("--playout-move-values", dict(type=float, nargs="?", const=0.25, default=0.0, metavar="TAU"),
                            "with --playout-value: MAST -- the playouts of a search learn a win rate per colour and point from "
                            "each other, and a point's weight in their draw is multiplied by exp((rate - 1/2) / TAU) (0.25 when "
                            "no value is given, with 16 virtual plays and counts halved at 16384: plausible and untuned; "
                            "default 0: off, DESIGN 30)"),
}
LATE = ("playout_move_contexts", "playout_move_values", "playout_reply_pairs", "playout_replies")   # the fields that are none of the constructor's


@dataclasses.dataclass
class PlayoutOptions:
    playout_value: int = 0              # N > 0: the value of a leaf is the share of N playouts its side to move wins
    playout_seed: int = 0
    playout_rules: str = "device"       # "host": the playouts on the host rules, the same bits
    playout_patterns: object = None     # None: uniformly random playouts
    playout_tactics: object = None      # None: no tactical weights
    playout_prior: float = 0.0          # 0: the priors are the policy net's alone
    playout_rave: float = 0.0           # 0: no RAVE
    playout_criticality: float = 0.0    # 0: the prior is AMAF's alone
    playout_pattern_prior: float = 0.0  # 0: no pattern term in the prior
    prior_patterns: object = None       # the tables of that term; None: the playouts' own
    prior_tactics: object = None
    # 0: no move-context table, else its temperature tau; in playout_move_values' form, and in front of it so that
    # the order of the fields before and the last three are what they were.
    playout_move_contexts: float = dataclasses.field(default=0.0, init=False)
    # 0: no move-value table, else its temperature tau; in playout_replies' form, and in front of the two reply
    # fields so that the order of the fields before and the last two are what they were.
    playout_move_values: float = dataclasses.field(default=0.0, init=False)
    # False: no replies keyed by the last two moves; in playout_replies' form, and in front of it so that the
    # order of the fields before and the last field are what they were.
    playout_reply_pairs: bool = dataclasses.field(default=False, init=False)
    # False: no reply table.  The last field, and none of the constructor's: its default lives on the class, so a
    # record built without it has the instance attributes (vars()) it had before the option existed, which NativeMCTS copies
    # onto itself; from_args and from_keywords set it, and so may a caller (opts.playout_replies = True).
    playout_replies: bool = dataclasses.field(default=False, init=False)

    TABLES = ("playout_patterns", "playout_tactics", "prior_patterns", "prior_tactics")

    def given(self, field):
        """A table is given when it is not None (it may be an array), a number when it is not 0."""
        x = getattr(self, field)
        return x is not None if field in self.TABLES else bool(x)

    @staticmethod
    def add_arguments(parser, rave=True, replies=True):
        """rave=False, replies=False: a front end whose one evaluator serves many games at once (selfplay) takes neither --
        there are no per-game RAVE records there, and the games would mix their reply tables.  selfplay has two flags of
        its own instead, --game-rave and --game-replies (RAVE records and a reply table per game), and
        --game-reply-pairs (a pair reply table per game).  The move-value table goes with the reply tables: one
        per search, so not where one evaluator serves many games; selfplay's own --game-move-values keeps one per game
        (DESIGN 31)."""
        for field, (flag, kw, text) in FLAGS.items():
            if (rave or field != "playout_rave") and (replies or field not in LATE):
                if field == "playout_value" and not (rave and replies):
                    text += "; RAVE and last-good-reply tables are per game here: --game-rave, --game-replies, --game-reply-pairs"
                parser.add_argument(flag, help=text, **kw)

    @classmethod
    def from_args(cls, parser, args):
        """The record of a parsed command line; a refused combination ends in parser.error, which names the flag."""
        self = cls(**{f: getattr(args, f) for f in FLAGS if hasattr(args, f) and f not in LATE})
        for f in LATE:
            if hasattr(args, f):
                setattr(self, f, type(getattr(cls, f))(getattr(args, f)))
        self.check(lambda field: FLAGS[field][0], lambda kind, text: parser.error(text), command_line=True)
        return self

    @classmethod
    def from_keywords(cls, kwargs):
        """The record of NativeMCTS's keywords (None or 0: not set): a missing prerequisite is a TypeError, a value out of
        range a ValueError."""
        def fail(kind, text):
            raise kind(text)

        self = cls(int(kwargs.get("playout_value") or 0), int(kwargs.get("playout_seed", 0)), kwargs.get("playout_rules", "device"),
                   kwargs.get("playout_patterns"), kwargs.get("playout_tactics"),
                   *(float(kwargs.get(f) or 0.0) for f in ("playout_prior", "playout_rave", "playout_criticality",
                                                            "playout_pattern_prior")),
                   kwargs.get("prior_patterns"), kwargs.get("prior_tactics"))
        self.playout_replies = bool(kwargs.get("playout_replies"))
        self.playout_reply_pairs = bool(kwargs.get("playout_reply_pairs"))
        self.playout_move_values = float(kwargs.get("playout_move_values") or 0.0)
        self.playout_move_contexts = float(kwargs.get("playout_move_contexts") or 0.0)
        self.check(str, fail)
        return self

    def check(self, name, fail, command_line=False):
        """The rules, once.  name(field) is what a message calls an option; fail(TypeError, text) reports a missing
        prerequisite and fail(ValueError, text) a value out of range."""
        value, prior = name("playout_value"), name("playout_prior")
        if self.playout_value < 0:
            fail(ValueError, f"{value} must not be negative")
        for field in ("playout_move_values", "playout_move_contexts"):       # (before `given`: a NaN is truthy)
            if not 0.0 <= getattr(self, field) < float("inf"):
                fail(ValueError, f"{name(field)} must be a finite number, 0 or more")
        for field in ("playout_patterns", "playout_tactics", "playout_prior", "playout_rave", "playout_replies",
                      "playout_reply_pairs", "playout_move_values", "playout_move_contexts"):
            if self.given(field) and not self.playout_value:
                fail(TypeError, f"{name(field)} goes with the playouts of {value}: it needs {value}")
        if self.playout_move_contexts and self.playout_move_values:
            fail(TypeError, f"{name('playout_move_contexts')} contains the move-value table (its plane 81): it goes without "
                            f"{name('playout_move_values')}")
        if not 0.0 <= self.playout_prior <= 1.0:
            fail(ValueError, f"{prior} must be within 0..1")
        for field in ("playout_rave", "playout_criticality", "playout_pattern_prior"):
            if not 0.0 <= getattr(self, field) < float("inf"):
                fail(ValueError, f"{name(field)} must be a finite number, 0 or more")
        for field in ("playout_criticality", "playout_pattern_prior"):
            if self.given(field) and not self.playout_prior:
                fail(TypeError, f"{name(field)} is a term of the playout prior: it needs {prior}")
        # The tables of the pattern term need the prior they are a term of.  A command line is stricter: there a table
        # without --playout-pattern-prior can only be a slip, while a caller of NativeMCTS may keep its tables in place
        # and switch the term on and off with playout_pattern_prior alone.
        needed = "playout_pattern_prior" if command_line else "playout_prior"
        for field in ("prior_patterns", "prior_tactics"):
            if self.given(field) and not self.given(needed):
                fail(TypeError, f"{name(field)} is a table of {name('playout_pattern_prior')}: it needs {name(needed)}")
        if self.playout_pattern_prior and not any(self.given(f) for f in self.TABLES):
            fail(ValueError, f"{name('playout_pattern_prior')} needs a table: " + ", ".join(name(f) for f in self.TABLES))

    def search_keywords(self):
        """The keywords of NativeMCTS / NativeGTP: the options that are set, and no others."""
        more = {f: getattr(self, f) for f in ("playout_value", "playout_patterns", "playout_tactics", "playout_prior",
                                              "playout_rave", "playout_criticality", "playout_replies",
                                              "playout_reply_pairs", "playout_move_values", "playout_move_contexts")
                if self.given(f)}
        if self.playout_pattern_prior:
            more.update(playout_pattern_prior=self.playout_pattern_prior, prior_patterns=self.prior_patterns,
                        prior_tactics=self.prior_tactics)
        return more

    def evaluator_keywords(self):
        """The keywords of rollout.PlayoutEvaluator after the engine: the options that are set, and no others."""
        more = {k: getattr(self, f) for k, f in (("prior", "playout_prior"), ("patterns", "playout_patterns"),
                                                 ("tactics", "playout_tactics"), ("criticality", "playout_criticality"))
                if self.given(f)}
        if self.playout_rave:
            more["rave"] = True
        if self.playout_replies or self.playout_reply_pairs:
            more["replies"] = 2 if self.playout_reply_pairs else True        # pairs contain singles
        if self.playout_move_values:
            more["move_values"] = self.playout_move_values
        if self.playout_move_contexts:
            more["move_contexts"] = self.playout_move_contexts
        if self.playout_pattern_prior:
            more.update(pattern_prior=self.playout_pattern_prior, prior_patterns=self.prior_patterns,
                        prior_tactics=self.prior_tactics)
        return dict(playouts=self.playout_value, seed=self.playout_seed, rules=self.playout_rules, **more)

    def name_suffix(self):
        """-mc64, then -pat with a playout table, -amaf, -rave, -crit, -pp with their parameters for the terms that are on, and
        -lgr with the reply table, -lgr2 when it is keyed by the last two moves, -mast with the move-value table, -nast with the move-context table."""
        name = f"-mc{self.playout_value}" + ("-pat" if self.given("playout_patterns") or self.given("playout_tactics") else "")
        for tag, x in (("amaf", self.playout_prior), ("rave", self.playout_rave), ("crit", self.playout_criticality),
                       ("pp", self.playout_pattern_prior)):
            name += f"-{tag}{x:g}" if x else ""
        name += "-lgr2" if self.playout_reply_pairs else "-lgr" if self.playout_replies else ""
        return name + ("-mast" if self.playout_move_values else "") + ("-nast" if self.playout_move_contexts else "")
