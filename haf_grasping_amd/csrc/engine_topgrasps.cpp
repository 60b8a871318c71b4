// engine_topgrasps.cpp -- haf_top_grasps: ranked, suppressed grasp candidates of the last scored batch (include/hafgrasp.h).  The
// device pass (topgrasps.hip) leaves every (cloud, roll)'s first D entries of its in-roll greedy sequence; this file merges the rolls
// of each cloud in key order with the cross-roll rule and the pose of haf_roll_pose.  The run-list scratch and the output block
// [hdr: 4 ints per (cloud, roll)][TopCandDev x depth per (cloud, roll)] are the ones every call outside the request path shares
// (call_scratch, call_io); a re-run with a larger depth asks for them again.  Built with -ffp-contract=off.
#include "engine_state.h"

namespace haf_host {

// steps 4-6 over one cloud's per-roll sequences (ascending roll order).  *need_more: a roll's present entries were used up while its
// sequence may go on and fewer than k candidates are kept -- the caller redoes the device pass with a larger depth (nothing in out
// is final then).
int top_merge(const haf_config &c, const haf_grasp_input *in, const std::vector<TopList> &lists, int k, int roll_window, double min_dist_m,
              haf_grasp_candidate *out, int32_t *n_found, bool *need_more, std::string &error)
{
    *n_found = 0;
    *need_more = false;
    const bool circular = (long)c.n_rolls * c.roll_step_deg == 180;
    const bool cross = roll_window > 0 && min_dist_m > 0.0;
    const double d2max = min_dist_m * min_dist_m;
    std::vector<int> pos(lists.size(), 0);
    int kept = 0;
    while (kept < k) {
        int best = -1;
        for (size_t i = 0; i < lists.size(); i++) {
            const TopList &l = lists[i];
            if (pos[i] >= l.n) {
                if (l.more) { *need_more = true; return HAF_OK; }
                continue;
            }
            if (best < 0) { best = (int)i; continue; }
            const TopList &b = lists[(size_t)best];
            const int v = l.rec[pos[i]].vote, bv = b.rec[pos[(size_t)best]].vote;
            if (v > bv || (v == bv && l.roll < b.roll)) best = (int)i;           // vote desc, then roll asc
        }
        if (best < 0) break;
        const TopList &l = lists[(size_t)best];
        const int j = pos[(size_t)best]++;
        haf_grasp_candidate cand;
        memset(&cand, 0, sizeof cand);
        const int rc = candidate_pose_impl(c, in, l.rec[j], l.roll, &cand.grasp, error);
        if (rc != HAF_OK) return rc;
        cand.run_length = l.len[j];
        cand.h_locmax = l.rec[j].h_locmax;
        bool drop = false;
        for (int q = 0; cross && q < kept && !drop; q++) {
            const haf_grasp_output &o = out[q].grasp;
            if (o.best_roll == l.roll) continue;
            int dr = std::abs(o.best_roll - l.roll);
            if (circular) dr = std::min(dr, c.n_rolls - dr);
            if (dr < 1 || dr > roll_window) continue;
            const double dx = cand.grasp.averaged_grasp_point[0] - o.averaged_grasp_point[0];
            const double dy = cand.grasp.averaged_grasp_point[1] - o.averaged_grasp_point[1];
            const double dz = cand.grasp.averaged_grasp_point[2] - o.averaged_grasp_point[2];
            const double d2 = dx * dx + dy * dy + dz * dz;                        // left to right, unfused (-ffp-contract=off)
            drop = d2 <= d2max;
        }
        if (!drop) out[kept++] = cand;
    }
    *n_found = kept;
    return HAF_OK;
}

static int top_grasps_impl(haf_engine *e, const haf_top_params *p, haf_grasp_candidate *out, int32_t *n_found)
{
    if (!p || !out || !n_found) return fail(e, HAF_E_ARG, "haf_top_grasps: null argument");
    if (e->mdl.prob_mode) return fail(e, HAF_E_ARG, "haf_top_grasps: not available with HAF_FLAG_PROBABILITY (fp32 votes)");
    const LastCall &last = e->last;
    if (last.B < 1 || last.R < 1 || (int)last.inputs.size() < last.B) return fail(e, HAF_E_ARG, "haf_top_grasps: no scored batch");
    if (p->k < 1 || p->k > 1024) return fail(e, HAF_E_ARG, "haf_top_grasps: k must be in [1, 1024]");
    if (p->min_vote < 1) return fail(e, HAF_E_ARG, "haf_top_grasps: min_vote must be >= 1");
    if (p->cell_radius < 0) return fail(e, HAF_E_ARG, "haf_top_grasps: cell_radius must be >= 0");
    if (p->roll_window < 0) return fail(e, HAF_E_ARG, "haf_top_grasps: roll_window must be >= 0");
    if (!(p->min_dist_m >= 0.0)) return fail(e, HAF_E_ARG, "haf_top_grasps: min_dist_m must be >= 0 (and not NaN)");
    const haf_config &c = e->cfg;
    const int H = c.grid_h, W = c.grid_w, B = last.B, R = last.R, BR = B * R;
    const size_t HW = (size_t)H * W;
    // the depth of the device pass: k entries per roll first, doubled while a roll's sequence runs out too early (testing build:
    // HAF_TOP_DEPTH sets the first depth, to drive the re-run).  A depth of H*W covers every run of a grid.
    long depth = p->k;
    if (const char *s = test_env("HAF_TOP_DEPTH")) depth = std::max(1L, atol(s));
    depth = std::min<long>(depth, (long)HW);
    // scratch: one slot of 2 x H*W words per workgroup; as many slots as (cloud, roll)s, up to 1024 and 2 GiB (every (cloud, roll) of
    // a C5 request at once: 288 x 4 MiB), the workgroups loop over the rest
    const size_t slot_words = HW;
    const int n_slots = (int)std::max<size_t>(1, std::min<size_t>({(size_t)BR, 1024, ((size_t)2 << 30) / (2 * slot_words * 8)}));
    const size_t hdr_bytes = (size_t)BR * 4 * sizeof(int);      // 16-byte aligned: TopCandDev follows
    std::vector<haf_grasp_candidate> res((size_t)B * p->k);
    std::vector<int32_t> found((size_t)B, 0);
    std::vector<haf_roll_record> rec;
    std::vector<int32_t> len;
    for (;;) {
        const size_t out_bytes = hdr_bytes + (size_t)BR * depth * sizeof(TopCandDev);
        CallBuffers cb;
        if (const int rc = call_buffers(e, "haf_top_grasps: ", out_bytes, "the output block", (size_t)n_slots * 2 * slot_words * sizeof(unsigned long long),
                                        "the run-list scratch", &cb)) return rc;
        int *d_hdr = reinterpret_cast<int *>(cb.dev);
        TopCandDev *d_cand = reinterpret_cast<TopCandDev *>(cb.dev + hdr_bytes);
        Dims d{};
        d.H = H; d.W = W; d.R = R; d.B = B;
        launch_top_grasps(e->d_ev16.p, reinterpret_cast<const float *>(e->d_heights.p), e->d_rec.p, reinterpret_cast<unsigned long long *>(cb.scratch), slot_words,
                          n_slots, d_hdr, d_cand, (int)depth, p->min_vote, p->cell_radius, d, cb.stream);
        if (const int rc = call_finish(e, cb, out_bytes)) return rc;
        const int *hdr = reinterpret_cast<const int *>(cb.host);
        const TopCandDev *hc = reinterpret_cast<const TopCandDev *>(cb.host + hdr_bytes);
        bool again = false;
        for (int b = 0; b < B && !again; b++) {
            found[(size_t)b] = 0;
            if ((int)last.inputs[(size_t)b].max_calculation_time < 0) continue;      // the reference scores none of its rolls
            size_t total = 0;
            for (int r = 0; r < R; r++) total += (size_t)hdr[4 * (b * R + r)];
            rec.resize(total);
            len.resize(total);
            std::vector<TopList> lists((size_t)R);
            size_t at = 0;
            for (int r = 0; r < R; r++) {
                const int br = b * R + r, n = hdr[4 * br];
                TopList &l = lists[(size_t)r];
                l.roll = last.roll_first + r;
                l.n = n;
                l.more = hdr[4 * br + 1] != 0;
                l.rec = rec.data() + at;
                l.len = len.data() + at;
                for (int i = 0; i < n; i++, at++) {
                    const TopCandDev &q = hc[(size_t)br * depth + i];
                    rec[at].vote = q.vote; rec[at].row = q.row; rec[at].col = q.col; rec[at].h_locmax = q.h_locmax;
                    rec[at].n_evals = hdr[4 * br + 2];
                    len[at] = q.len;
                }
            }
            bool need_more = false;
            const int rc = top_merge(c, &last.inputs[(size_t)b], lists, p->k, p->roll_window, p->min_dist_m, res.data() + (size_t)b * p->k,
                                     &found[(size_t)b], &need_more, e->error);
            if (rc != HAF_OK) return rc;
            again = need_more;
        }
        if (!again) break;
        if (depth >= (long)HW) return fail(e, HAF_E_INTERNAL, "haf_top_grasps: a roll's sequence outgrew its grid");
        depth = std::min<long>(2 * depth, (long)HW);
    }
    memcpy(out, res.data(), res.size() * sizeof(haf_grasp_candidate));
    memcpy(n_found, found.data(), found.size() * sizeof(int32_t));
    return HAF_OK;
}

}  // namespace haf_host

extern "C" {

void haf_top_params_default(const haf_engine *e, haf_top_params *p)
{
    if (!p) return;
    haf_config dc;
    haf_config_default(&dc);
    p->k = 8;
    p->min_vote = (e ? e->cfg.graspval_th : dc.graspval_th) + 1;      // the hypothesis threshold (server.cpp:960-962)
    p->cell_radius = 7;
    p->roll_window = 1;
    p->min_dist_m = 0.02;
}

int haf_top_grasps(haf_engine *e, const haf_top_params *p, haf_grasp_candidate *out, int32_t *n_found)
{
    if (!e) return HAF_E_ARG;
    return guarded(&e->error, [&] { return top_grasps_impl(e, p, out, n_found); });
}

}  // extern "C"
