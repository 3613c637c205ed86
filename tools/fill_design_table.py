"""Rewrite the measured table of DESIGN.md section 4 (between the R6_TABLE markers) from profiles/r06_bench_line.json and its companions."""
import json, os, re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
d = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_line.json")))
g = json.load(open(os.path.join(ROOT, "profiles", "r06_bench_line_generator_bench.json")))
c5 = {k: json.load(open(os.path.join(ROOT, "profiles", f"r06_bench_cfg5_{k}_line.json"))) for k in ("200k", "1M", "1M_f64")}
r, c, st, cb, w, pm = d["roofline"], d["config"], d["config"]["stage_ms"], d["cpu_baseline"], d["extra"]["D_reference_defaults_nrndm3000"], d["precision_modes"]
tel = d["telemetry"]
pw = lambda t: t.get("Current Socket Graphics Package Power (W)", "?")
tj = lambda t: t.get("Temperature (Sensor junction) (C)", "?")
tab = f"""<!-- R6_TABLE_BEGIN (tools/fill_design_table.py) -->
| line (one box, `python bench.py --full --gpus 1 --steps 20 --warmup 5`; `profiles/r06_bench_line.json`) | value |
|---|---|
| **headline: cells/s through A → B → (C) → D, f64, uint16 layers, survey dataset** | **{d['value']/1e3:.1f} k cells/s** ({d['ms_per_step']:.1f} ms per pass) |
| the same on the dataset of rounds 1-5 (`--generator bench`, `r06_bench_line_generator_bench.json`; round 5's builder line: 197.6-202 k) | {g['value']/1e3:.1f} k cells/s (stage D {g['config']['stage_ms']['D_coldeltacor']:.1f} ms) |
| stages | A {st['A_knn_imputation']:.1f} ms (kNN search {c['A_knn_search_ms']:.2f} + pooling {c['A_pooling_ms']:.2f}), B {st['B_fit_slope']:.2f}, C folded, D {st['D_coldeltacor']:.1f} |
| `roofline` (stage D, VALU issue) | achieved {r['achieved']:.0f} Ginstr/s of {r['peak']:.0f}: `frac` **{r['frac']:.3f}**; {r['frac_of_f64_issue_peak']:.2f} of the f64 issue peak; {r['frac_of_mix_floor']:.2f} of the element mix's issue time ({r['frac_of_mix_floor_at_effective_clock']:.2f} at the {r['effective_clock_ghz']:.2f} GHz measured in the run; per XCD {min(r['effective_clock']['per_xcd_mean']):.2f}-{max(r['effective_clock']['per_xcd_mean']):.2f}); {r['profile_valu_insts_per_pair_chunk']:.1f} VALU instructions per pair-chunk |
| `traffic` (PMC passes) | {r['traffic']/1e9:.0f} GB per launch = {r['hbm_frac_measured']:.2f} of the HBM peak; §8(d)'s no-reuse byte model over launch time: {r['vs_noreuse_model']:.2f} × peak (rows shared out of LDS and L2) |
| A pooling / B by algorithmic bytes | {d['stages']['A_pooling']['frac']:.2f} / {d['stages']['B_fit_slope']['frac']:.2f} of the HBM peak |
| `cpu_baseline` (kind `{cb['kind']}`, {cb['cores']} threads of the GPU box's host) | {cb['value']:.1f} cells/s (stage D by the reference's own compiled kernel at full width) |
| f32 production mode / f32 literal rule (`precision_modes`) | {pm['f32_production']['cells_per_s']/1e3:.0f} k / {pm['f32_literal_rule']['cells_per_s']/1e3:.0f} k cells/s (stage D {pm['f32_production']['D_ms']:.1f} / {pm['f32_literal_rule']['D_ms']:.1f} ms) |
| D at the reference's default list width (nrndm = 3000) | {w['ms']/1e3:.2f} s = {w['cells_per_s']/1e3:.1f} k cells/s; `frac` {w['roofline']['frac']:.3f}, {w['roofline']['frac_of_f64_issue_peak']:.2f} of the f64 issue peak, {w['roofline']['frac_of_mix_floor']:.2f} of its mix floor; HBM {w['roofline']['hbm_frac_measured']:.2f} of peak |
| randomised control in the same launch | {c['D_dual_control_over_single']:.2f} × a single launch |
| E `calculate_embedding_shift` / F `prepare_markov` / `run_markov` per step / default `fit_gammas` (facade, f64) | {c['E_calculate_embedding_shift_ms']:.1f} ms / {c['F_prepare_markov_ms']:.1f} ms / **{c['F_run_markov_ms_per_step']:.2f} ms** (round 5: 0.79) / {c['B_fit_gammas_default_ms']:.1f} ms |
| cfg2 (10 000 × 20 000, A + B) | unbalanced {c['cfg2_unbalanced_A_ms']:.1f} + {c['cfg2_unbalanced_B_ms']:.2f} ms; balanced {c['cfg2_balanced_A_ms']:.1f} + {c['cfg2_balanced_B_ms']:.2f} ms |
| cfg5 (1 000 000 × 30 000 CSR on one GPU, `profiles/r06_bench_cfg5_*`) | {c5['1M']['value']/1e3:.0f} k cells/s in f32 ({c5['1M']['ms_per_step']/1e3:.2f} s per pass), {c5['1M_f64']['value']/1e3:.0f} k in f64 ({c5['1M_f64']['ms_per_step']/1e3:.2f} s); 200 000 cells: {c5['200k']['value']/1e3:.0f} k (f32) |
| all-pairs linear kernel incl. its repair launch (10 000 × 20 000, `profiles/r06_full_kernels.txt`) | 120.5-121.5 ms f64 / 118 ms f32 storage = 0.84 / 0.86 of the f64 matrix peak; kNN-pooled matrices 127 ms |
| GPU suite from the repository root | 353 passed in 332 s; `smoke()` ok against the oracle and the reference's own kernel (1.1e-15) |

Box-to-box, now with the telemetry beside it: the same binary gave stage D = 217.4 ms (206 k cells/s) on one box of this round - shader clock under
stage D 2.37 GHz (per XCD 2.35-2.39), 841 W / 46 °C before the timed steps - and 229-232 ms on others - 2.30-2.32 GHz, 895-901 W / 48-50 °C
(`profiles/r06_generators_two_boxes.txt` and this run: {pw(tel['smi_before_timed_steps'])} W / {tj(tel['smi_before_timed_steps'])} °C before, {tj(tel['smi_after_timed_steps'])} °C after).  The boxes that draw more power for the same work hold a 2-3 % lower clock:
that explains about half of the 5-6 % spread; fabric and memory clocks are the same (1250 / 2000 MHz), the rest is still unexplained.
<!-- R6_TABLE_END -->"""
p = os.path.join(ROOT, "DESIGN.md")
s = open(p).read()
if "<!-- R6_TABLE_BEGIN" in s:
    s = re.sub(r"<!-- R6_TABLE_BEGIN.*?<!-- R6_TABLE_END -->", lambda m: tab, s, flags=re.S)
else:
    a = s.index("| line (one box, `python bench.py --full --gpus 1 --steps 20 --warmup 5`")
    b = s.index("## 5. Parity")
    s = s[:a] + tab + "\n\n" + s[b:]
open(p, "w").write(s)
print("DESIGN.md table rewritten:", d["value"], g["value"])
