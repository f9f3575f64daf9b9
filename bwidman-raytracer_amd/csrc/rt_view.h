// rt_view.h — what the host knows about the view the context is in and about
// what was computed for a view: the view counter, the validity of the first-hit
// guides, the roles of the two temporal history sets (rt_temporal,
// rt_temporal_var, rt_render_adaptive_reprojected) and the record of the
// assembled frame (rt_assemble*).  Plain C++, no HIP.  rt_context holds one
// rt_view_state; only the transitions below assign its fields, and every unit
// asks its questions through the queries.  The buffers the state speaks about
// (the guides, TpSet::{col, ga, gb, mom} with the sets' cameras,
// Assembled::{sum, mom, cnt}) and the passes stay in the context.
//
// Fields: the view counter (a view is one scene, camera and frame shape); the
// guides' validity; of the two history sets, which one is the history (the
// other takes the pending result), whether a history and a pending result
// exist, the view the pending result was made in, the frame shape of both sets
// and whether each set carries {s2, dof} per pixel (rt_temporal_var wrote it);
// the assembled frame's record: made, the view and shape it was made in, its
// plane count, and the n and J it stands for.
//
//   event                                  effect
//   rt_set_scene (on success)              new view; history and pending dropped (primitive ids
//                                          change meaning)
//   rt_set_camera, moving rt_controls      new view; nothing else
//   rt_init_rand (explicit or implicit)    new view; the sets take the frame shape: history and
//                                          pending dropped if it differs from theirs
//   temporal call, after its checks and    the sets take the frame shape (as above); then a result
//   allocations                            pending from an earlier view becomes the history: the
//                                          sets swap roles
//   temporal result stored                 pending = this view; the set has moments as its writer says
//   rt_temporal_reset                      history and pending dropped
//   guides computed                        valid until the next new view
//   assembly, before its pass is queued    not made
//   assembly queued                        the full record, stamped with the view and the frame shape
//   rt_assemble_drop                       not made
//   an assembly buffer lost in a failed    not made
//   growth
//
// A new view invalidates the guides and nothing else: the pending result and
// the assembled frame carry the view they were made in, and the queries compare.
// A render of another frame shape drops the history through its implicit
// rt_init_rand, as the table says.
//
// rt_init_rand and the start of a temporal call share one transition,
// set_shape.  Before this header rt_init_rand compared with the sets' shape and
// dropped without taking the new one; only a temporal call took it.  Taking it
// early changes no later answer: a role (history, pending) is only ever set by
// a temporal call, which takes the shape first, so "a role is set" implies "the
// sets' shape is the shape of that call" under either rule; and while no role is
// set, dropping does nothing and every query that reads the shape (pending_current)
// asks for a pending result first.  tests/view_trace.py is the check.
#pragma once

class rt_view_state {
public:
    // the non-buffer record of the assembled frame (DESIGN.md sections 17 and 19)
    struct Assembled {
        bool made = false;
        unsigned long long view = 0;
        int width = 0, height = 0;
        int planes = 0;                    // of the blocks it was made from (rt_block_shape_of: what they hold)
        unsigned frames = 0, batches = 0;  // n and J (0 without moments); of a counted frame the uniform base
    };

private:
    unsigned long long view_ = 1;
    bool guides_valid_ = false;
    int hist_ = 0;  // the history set; the other one takes the pending result
    bool has_hist_ = false, has_pending_ = false;
    unsigned long long pending_view_ = 0;
    int tp_w_ = 0, tp_h_ = 0;  // frame shape of both sets
    bool has_mom_[2] = {false, false};
    Assembled as_;

public:
    // ---- queries ---------------------------------------------------------------
    bool guides_valid() const { return guides_valid_; }
    int history_set() const { return hist_; }
    int pending_set() const { return hist_ ^ 1; }
    bool has_history() const { return has_hist_; }
    bool history_has_moments() const { return has_mom_[hist_]; }
    // a pending result of this view and of a width x height frame exists; whether it carries moments
    bool pending_current(int width, int height) const {
        return has_pending_ && pending_view_ == view_ && tp_w_ == width && tp_h_ == height;
    }
    bool pending_has_moments() const { return has_mom_[hist_ ^ 1]; }
    // made, and neither the view nor the frame shape changed since
    bool assembled_current(int width, int height) const {
        return as_.made && as_.view == view_ && as_.width == width && as_.height == height;
    }
    const Assembled& assembled() const { return as_; }  // (made: current or stale)

    // ---- transitions -----------------------------------------------------------
    void new_view() {
        guides_valid_ = false;
        view_++;
    }
    void guides_computed() { guides_valid_ = true; }
    void drop_history() { has_hist_ = has_pending_ = false; }
    void set_shape(int width, int height) {
        if (width == tp_w_ && height == tp_h_) return;
        drop_history();
        tp_w_ = width;
        tp_h_ = height;
    }
    // The swap is of host-side roles only: the caller's stream waits order the
    // call's kernel after every earlier reader of the set it now writes.
    void temporal_start(int width, int height) {
        set_shape(width, height);
        if (!has_pending_ || pending_view_ == view_) return;
        hist_ ^= 1;
        has_hist_ = true;
        has_pending_ = false;
    }
    void temporal_stored(bool has_mom) {
        has_mom_[hist_ ^ 1] = has_mom;
        has_pending_ = true;
        pending_view_ = view_;
    }
    void assembled_drop() { as_.made = false; }
    void assembled_done(int width, int height, int planes, unsigned frames, unsigned batches) {
        as_ = {true, view_, width, height, planes, frames, batches};
    }
};
