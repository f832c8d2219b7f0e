/*
 * One seeded C-API trial with every time-weighted statistic on: an
 * object queue, a resource, a resource pool and a buffer all record.
 * Prints the four stats vectors (mean, sd, min, max) as hex floats, so
 * the output is exact; tests/test_hot_shrink.py compares it with the
 * recorded output under tests/golden/.
 */
#include <cimba.h>

#include <stdio.h>

#define NUM_JOBS 3000u

struct ctx {
    cmb_objectqueue* queue;
    cmb_resource* server;
    cmb_resourcepool* tools;
    cmb_buffer* stock;
    uint64_t i;
    void* obj;
    uint64_t served;
};

static void arrival_body(cmb_sim* sim, cmb_process* me, void* vctx) {
    struct ctx* c = vctx;
    CMB_PROC_BEGIN(sim, me);
    for (c->i = 0; c->i < NUM_JOBS; c->i++) {
        CMB_HOLD(sim, me, cmb_random_exponential(sim, 1.25));
        CMB_OBJECTQUEUE_PUT(sim, me, c->queue, (void*)(uintptr_t)(c->i + 1));
        CMB_BUFFER_PUT(sim, me, c->stock, 3);
    }
    CMB_PROC_END(sim, me);
}

static void server_body(cmb_sim* sim, cmb_process* me, void* vctx) {
    struct ctx* c = vctx;
    CMB_PROC_BEGIN(sim, me);
    for (;;) {
        CMB_OBJECTQUEUE_GET(sim, me, c->queue, &c->obj);
        if (CMB_SIGNAL(sim, me) != CMB_PROCESS_SUCCESS) break;
        CMB_RESOURCE_ACQUIRE(sim, me, c->server);
        CMB_RESOURCEPOOL_ACQUIRE_ALL(sim, me, c->tools, 2);
        CMB_BUFFER_GET(sim, me, c->stock, 2);
        CMB_HOLD(sim, me, cmb_random_exponential(sim, 1.0));
        cmb_resourcepool_release(sim, c->tools, me, 2);
        cmb_resource_release(sim, c->server, me);
        c->served++;
    }
    CMB_PROC_END(sim, me);
}

static void show(const char* what, const double st[4]) {
    printf("%s %a %a %a %a\n", what, st[0], st[1], st[2], st[3]);
}

static void run_trial(cmb_sim* sim, void* vout) {
    struct ctx c = {0};
    double st[4];
    (void)vout;

    c.queue = cmb_objectqueue_create(sim);
    cmb_objectqueue_initialize(sim, c.queue, "Jobs", 64);
    cmb_objectqueue_recording_start(sim, c.queue);
    c.server = cmb_resource_create(sim);
    cmb_resource_initialize(sim, c.server, "Server");
    cmb_resource_recording_start(sim, c.server);
    c.tools = cmb_resourcepool_create(sim);
    cmb_resourcepool_initialize(sim, c.tools, "Tools", 3);
    cmb_resourcepool_start_recording(sim, c.tools);
    c.stock = cmb_buffer_create(sim);
    cmb_buffer_initialize(sim, c.stock, "Stock", 1000000, 10);
    cmb_buffer_recording_start(sim, c.stock);

    cmb_process* a = cmb_process_spawn(sim, "Arrival", arrival_body, &c, 0);
    cmb_process* s = cmb_process_spawn(sim, "Server", server_body, &c, 0);
    cmb_process_start(sim, a);
    cmb_process_start(sim, s);
    cmb_event_queue_execute(sim);

    printf("served %llu t %a\n", (unsigned long long)c.served, cmb_time(sim));
    cmb_objectqueue_stats(sim, c.queue, st);
    show("queue", st);
    cmb_resource_stats(sim, c.server, st);
    show("resource", st);
    cmb_resourcepool_stats(sim, c.tools, st);
    show("pool", st);
    cmb_buffer_stats(sim, c.stock, st);
    show("buffer", st);
    cmb_resourcepool_print_report(sim, c.tools, stdout);
}

int main(void) {
    int dummy = 0;
    return (int)cimba_run(&dummy, 1, sizeof(dummy), run_trial, 0x5eedULL, 1);
}
