// rt_accum.h — what the host knows about the accumulation in frameSum: the
// frame counter, the luminance moment tracking (rt_set_moments) and the
// non-uniform state of adaptive sampling (rt_render_adaptive).  Plain C++, no
// HIP.  rt_context holds one rt_accum_state; only the transitions below assign
// its fields, and every unit asks its questions through the queries.
//
// Fields: frame (the next uniform render's first frame; frame - 1 frames are
// accumulated), the tracking switch, live / batches / next (tracking follows
// the accumulation, over `batches` render calls, up to frame next - 1), the
// non-uniform flag (the context's ad_cnt holds {n_p, J_p} per pixel) with
// max_n >= every n_p, the filter switch (rt_set_adaptive_filters), and the
// radius of the current row-sum export (rt_adaptive_export_rows, the first
// phase of an adaptive call on row shards; -1: none).
//
//   event                                  effect
//   rt_set_scene (on success)              frame 1; non-uniform ends; tracking untouched
//   rt_set_camera, moving rt_controls      frame 1; nothing else
//   rt_reset_accumulation                  frame 1; nothing else
//   rt_init_rand (explicit or implicit)    tracking ends (batches 0) and non-uniform ends, before
//                                          the buffers are touched; frame 1 on success
//   rt_set_state(fc)                       frame fc; tracking and non-uniform end
//   rt_set_moments(x), x != the switch     tracking and non-uniform end; switch = x
//   uniform render, before it is queued    1. first = first_frame ? first_frame : frame
//                                          2. non-uniform and first != 1: refused, nothing changes;
//                                             non-uniform and first == 1: it becomes uniform
//                                          3. first + samples must fit the frame counter
//                                          4. track = switch && (first == 1 || (live && first == next));
//                                             not track: tracking ends
//                                          5. the moment buffers cannot be allocated: tracking ends
//   uniform render done                    frame = first + samples; if tracked: batches =
//                                          (first == 1 ? 1 : batches + 1), live, next = first + samples
//   launch failure                         tracking and non-uniform end; frame unchanged
//   adaptive call, before it is queued     needs batches >= 2 (rt_render_adaptive_reprojected: >= 1)
//                                          and `current`, else refused
//   adaptive call done                     first of an accumulation: max_n = next - 1; then
//                                          max_n += samples; non-uniform; frame, batches, next unchanged
//   adaptive launch failure                tracking and non-uniform end
//   row-sum export done                    the export is current, with its radius; nothing else
//
// The row-sum export describes the moments and counts it was made from: it ends
// with every restart (scene, camera, reset), with the tracking, with a uniform
// render that is not refused and with an adaptive call.
//
// "Tracking ends" always takes the non-uniform state with it: the counts go
// with the moments they belong to.  Between a restart (frame 1) and the next
// render the tracked state still describes the last tracked accumulation, as
// the readouts document; `current` is the question whether it also describes
// the accumulation the frame counter reports.
#pragma once

class rt_accum_state {
    unsigned frame_ = 1;
    bool switch_ = false, live_ = false;
    unsigned batches_ = 0, next_ = 0;
    bool nonuniform_ = false, filters_ = false;
    unsigned long long max_n_ = 0;
    int export_radius_ = -1;

public:
    // ---- queries ---------------------------------------------------------------
    unsigned frame() const { return frame_; }
    unsigned frames() const { return frame_ - 1u; }  // of the uniform base
    bool tracking() const { return switch_; }
    unsigned batches() const { return live_ ? batches_ : 0u; }  // J to report; 0 when not live
    unsigned tracked_frames() const { return next_ - 1u; }      // n behind the moments (while live)
    bool nonuniform() const { return nonuniform_; }
    bool filters() const { return filters_; }
    bool filters_refuse() const { return nonuniform_ && !filters_; }
    // the tracked moments describe the accumulation the context reports
    bool current() const { return live_ && next_ == frame_; }
    // no n_p exceeds it: what an adaptive call's `samples` must not carry past 2^32 - 1
    // (J_p <= n_p: a batch has at least one frame)
    unsigned long long adaptive_base() const { return nonuniform_ ? max_n_ : (unsigned long long)(next_ - 1u); }
    // the context's last row-sum export, made with `radius`, still describes the moments and counts
    bool export_current(int radius) const { return export_radius_ >= 0 && export_radius_ == radius && current(); }

    // ---- transitions -----------------------------------------------------------
    void restart() {
        frame_ = 1;
        export_radius_ = -1;
    }
    void end_nonuniform() { nonuniform_ = false; }
    void end_tracking() {
        live_ = false;
        batches_ = 0;
        nonuniform_ = false;
        export_radius_ = -1;
    }
    void set_frame(unsigned fc) {
        frame_ = fc;
        end_tracking();
    }
    void set_tracking(bool on) {
        if (on != switch_) end_tracking();
        switch_ = on;
    }
    void set_filters(bool on) { filters_ = on; }

    // a uniform render: steps 1 to 3, then step 4 (true: the call is tracked),
    // then its end (`tracked`: what step 4 said, unless step 5 ended it)
    enum class Start { ok, nonuniform, overflow };
    Start uniform_start(unsigned first_frame, int samples, unsigned& first) {
        first = first_frame ? first_frame : frame_;
        if (nonuniform_ && first != 1u) return Start::nonuniform;
        nonuniform_ = false;
        if ((unsigned long long)first + (unsigned)samples > 0xffffffffull) return Start::overflow;
        export_radius_ = -1;
        return Start::ok;
    }
    bool uniform_track(unsigned first) {
        const bool track = switch_ && (first == 1u || (live_ && first == next_));
        if (!track) end_tracking();
        return track;
    }
    void uniform_done(unsigned first, int samples, bool tracked) {
        frame_ = first + (unsigned)samples;  // Main.cu:480 accumulatedFrames++
        if (!tracked) return;
        batches_ = first == 1u ? 1u : batches_ + 1u;
        live_ = true;
        next_ = frame_;
    }
    void adaptive_done(int samples) {
        max_n_ = adaptive_base() + (unsigned)samples;
        nonuniform_ = true;
        export_radius_ = -1;
    }
    void export_done(int radius) { export_radius_ = radius; }
};
