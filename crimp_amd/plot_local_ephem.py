"""Plot local ephemerides (drop-in for CRIMP's ``plot_local_ephem.py``, v2.3.0; the ``localephemerides_plot``
script): F0 and F1 of every window against time, from the table ``get_local_ephem`` writes."""
import argparse

import pandas as pd


def read_local_ephemerides(localephem: str, t_start: float | None = None, t_end: float | None = None):
    """The local-ephemerides .txt table as a DataFrame, cut to [t_start, t_end] in TOA_MJD_ref and re-indexed."""
    df = pd.read_csv(localephem, sep=r"\s+", comment="#", header=0)
    ref = df["TOA_MJD_ref"]
    lo = ref.min() if t_start is None else t_start
    hi = ref.max() if t_end is None else t_end
    return df.loc[(ref >= lo) & (ref <= hi)].reset_index(drop=True)


def plot_local_ephemerides(local_df, glitches=None, plotname=None):
    """F0 (top) and F1 (bottom) with their uncertainties; the horizontal bars are the windows' half-spans, dashed
    red lines the glitch epochs. ``local_df`` has TOA_MJD_ref, TOA_MJD_ref_err, F0, F0_err, F1, F1_err. Shown, or
    saved as ``plotname``.pdf."""
    import matplotlib.pyplot as plt
    fig, axs = plt.subplots(2, 1, figsize=(10, 8), dpi=80, facecolor="w", edgecolor="k", sharex=True)
    panels = (("F0", r"$\,\mathrm{Frequency\ (Hz)}$", r"$F$"),
              ("F1", r"$\,\mathrm{\dot{F}\ (Hz\,s^{-1})}$", r"$\dot{F}$"))
    for ax, (col, ylabel, label) in zip(axs, panels):
        _, caps, bars = ax.errorbar(local_df["TOA_MJD_ref"], local_df[col], xerr=local_df["TOA_MJD_ref_err"],
                                    yerr=local_df[col + "_err"], fmt="o", color="k", ecolor="gray", elinewidth=1.5,
                                    capsize=2, markersize=6, label=label, alpha=0.7)
        for artist in list(bars) + list(caps):
            artist.set_alpha(0.35)
        ax.set_ylabel(ylabel, fontsize=14)
        ax.tick_params(axis="both", labelsize=14, width=1.5)
        ax.ticklabel_format(style="sci", axis="y", scilimits=(0, 0))
        ax.xaxis.offsetText.set_fontsize(14)
        ax.yaxis.offsetText.set_fontsize(14)
        ax.grid(True, linestyle="--", alpha=0.3)
        for g in (glitches if glitches is not None else ()):
            ax.axvline(g, color="red", linestyle="--", linewidth=1.5, alpha=0.7)
        for side in ("top", "bottom", "left", "right"):
            ax.spines[side].set_linewidth(1.5)
    axs[1].set_xlabel(r"$\,\mathrm{Time\ (MJD)}$", fontsize=14)
    fig.tight_layout()
    if plotname is None:
        plt.show()
    else:
        fig.savefig(str(plotname) + ".pdf", format="pdf", dpi=300, bbox_inches="tight")
        plt.close(fig)


def main(argv=None):
    p = argparse.ArgumentParser(description="Plot local ephemerides")
    p.add_argument("localephem", type=str,
                   help=".txt file of local ephemerides built with get_local_ephem.py or the localephemerides script")
    p.add_argument("-ts", "--t_start", help="Start from (MJD)", type=float, default=None)
    p.add_argument("-te", "--t_end", help="Stop at (MJD)", type=float, default=None)
    p.add_argument("-gl", "--glitches", help="MJDs of glitches (where dashed lines will be plotted)", type=float,
                   nargs="+", default=None)
    p.add_argument("-ep", "--ephem_plot", help="Plot of local ephemerides (default=None)", type=str, default=None)
    a = p.parse_args(argv)
    plot_local_ephemerides(read_local_ephemerides(a.localephem, a.t_start, a.t_end), glitches=a.glitches,
                           plotname=a.ephem_plot)


if __name__ == "__main__":
    main()
