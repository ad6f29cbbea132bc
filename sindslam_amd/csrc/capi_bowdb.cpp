// C ABI: key-frame database (include/sind_hip.h, "sind_bowdb_*").
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../include/sind_hip.h"
#include "match.hpp"

struct sind_bowdb {
    int device = 0, capSlots = 0, capWords = 0, maxQ = 0; hipStream_t stream = nullptr;
    long long nextSeq = 0; std::vector<long long> seq;                // per slot: the value of the counter at its add, -1 while dead
    bool slotsChanged = true;                                         // slotN.h is ahead of the device
    Staged<int> slotN; DevBuf<int> slotWord; DevBuf<double> slotValue;      // [capSlots] (-1: dead), [capSlots][capWords]
    Staged<int> qN, qWord, common, firstWord; Staged<double> qValue; Staged<float> score;      // [maxQ], [maxQ][capWords], outputs [maxQ][capSlots]
};

namespace {
// a BowVector as std::map iterates it: NULL only when empty, at most cap words, ids >= 0 and strictly ascending
int check_vector(const char* who, const int* word, const double* value, int n, int cap) {
    if (n < 0 || (n && (!word || !value))) { sind_set_error("%s: null array or negative count", who); return SIND_E_ARG; }
    if (n > cap) { sind_set_error("%s: %d words, capacity %d", who, n, cap); return SIND_E_CAPACITY; }
    for (int i = 0; i < n; i++) if (word[i] < 0 || (i && word[i] <= word[i - 1])) { sind_set_error("%s: word ids must be >= 0 and ascend strictly (entry %d)", who, i); return SIND_E_ARG; }
    return SIND_OK;
}
}  // namespace

extern "C" {

int sind_bowdb_create(int cap_slots, int cap_words, int max_queries, int device, sind_bowdb** out) {
    if (!out || cap_slots < 1 || cap_words < 1 || max_queries < 1) { sind_set_error("sind_bowdb_create: bad arguments"); return SIND_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    sind_bowdb* db = new sind_bowdb(); db->device = device; db->capSlots = cap_slots; db->capWords = cap_words; db->maxQ = max_queries;
    const size_t ns = cap_slots, nw = ns * cap_words, nq = (size_t)max_queries * cap_words, no = (size_t)max_queries * cap_slots;
    int r = SIND_OK;
    if ((r = db->slotN.alloc(ns)) || (r = db->slotWord.alloc(nw)) || (r = db->slotValue.alloc(nw)) || (r = db->qN.alloc(max_queries)) || (r = db->qWord.alloc(nq)) || (r = db->qValue.alloc(nq)) ||
        (r = db->common.alloc(no)) || (r = db->firstWord.alloc(no)) || (r = db->score.alloc(no))) { delete db; return r; }
    if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) { delete db; sind_set_error("sind_bowdb_create: stream creation failed"); return SIND_E_HIP; }
    db->seq.assign(ns, -1); std::fill(db->slotN.h.begin(), db->slotN.h.end(), -1);
    *out = db; return SIND_OK;
}

int sind_bowdb_destroy(sind_bowdb* db) {
    if (!db) return SIND_OK;
    (void)hipSetDevice(db->device);
    if (db->stream) (void)hipStreamSynchronize(db->stream);
    hipStream_t s = db->stream; delete db; if (s) (void)hipStreamDestroy(s);
    return SIND_OK;
}

int sind_bowdb_add(sind_bowdb* db, int slot, const int* word, const double* value, int n) {
    if (!db || slot < 0 || slot >= db->capSlots) { sind_set_error("sind_bowdb_add: bad arguments (slot %d of %d)", slot, db ? db->capSlots : 0); return SIND_E_ARG; }
    if (db->seq[slot] >= 0) { sind_set_error("sind_bowdb_add: slot %d is live", slot); return SIND_E_STATE; }
    SIND_TRY(check_vector("sind_bowdb_add", word, value, n, db->capWords));
    HIP_TRY(hipSetDevice(db->device));
    if (n) {
        const size_t o = (size_t)slot * db->capWords;
        HIP_TRY(hipMemcpyAsync(db->slotWord.p + o, word, (size_t)n * sizeof(int), hipMemcpyHostToDevice, db->stream));
        HIP_TRY(hipMemcpyAsync(db->slotValue.p + o, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice, db->stream));
        HIP_TRY(hipStreamSynchronize(db->stream));                    // the caller's arrays are free again on return
    }
    db->slotN.h[slot] = n; db->seq[slot] = db->nextSeq++; db->slotsChanged = true;
    return SIND_OK;
}

int sind_bowdb_erase(sind_bowdb* db, int slot) {
    if (!db || slot < 0 || slot >= db->capSlots) { sind_set_error("sind_bowdb_erase: bad arguments (slot %d of %d)", slot, db ? db->capSlots : 0); return SIND_E_ARG; }
    if (db->seq[slot] >= 0) { db->slotN.h[slot] = -1; db->seq[slot] = -1; db->slotsChanged = true; }      // erasing what is not there changes nothing, as in the reference
    return SIND_OK;
}

int sind_bowdb_clear(sind_bowdb* db) {
    if (!db) { sind_set_error("sind_bowdb_clear: bad arguments"); return SIND_E_ARG; }
    std::fill(db->seq.begin(), db->seq.end(), -1LL); std::fill(db->slotN.h.begin(), db->slotN.h.begin() + db->capSlots, -1); db->slotsChanged = true;
    return SIND_OK;
}

long long sind_bowdb_sequence(const sind_bowdb* db, int slot) { return (db && slot >= 0 && slot < db->capSlots) ? db->seq[slot] : -1; }

int sind_bowdb_query(sind_bowdb* db, const sind_bowdb_query_item* q, int Q) {
    if (!db || !q || Q < 1) { sind_set_error("sind_bowdb_query: bad arguments"); return SIND_E_ARG; }
    if (Q > db->maxQ) { sind_set_error("sind_bowdb_query: Q=%d, max_queries %d", Q, db->maxQ); return SIND_E_CAPACITY; }
    for (int i = 0; i < Q; i++) {
        if (!q[i].common || !q[i].first_word || !q[i].score) { sind_set_error("sind_bowdb_query: null output in query %d", i); return SIND_E_ARG; }
        SIND_TRY(check_vector("sind_bowdb_query", q[i].word, q[i].value, q[i].n, db->capWords));
    }
    HIP_TRY(hipSetDevice(db->device));
    const size_t cw = db->capWords, cs = db->capSlots;
    for (int i = 0; i < Q; i++) {
        db->qN.h[i] = q[i].n;
        if (q[i].n) { std::memcpy(&db->qWord.h[i * cw], q[i].word, (size_t)q[i].n * sizeof(int)); std::memcpy(&db->qValue.h[i * cw], q[i].value, (size_t)q[i].n * sizeof(double)); }
    }
    hipStream_t s = db->stream;
    if (db->slotsChanged) { SIND_TRY(db->slotN.up(cs, s)); db->slotsChanged = false; }
    SIND_TRY(db->qN.up(Q, s)); SIND_TRY(db->qWord.up(Q * cw, s)); SIND_TRY(db->qValue.up(Q * cw, s));
    const sind::BowDbArrays a{db->slotN.d.p, db->slotWord.p, db->slotValue.p, db->qN.d.p, db->qWord.d.p, db->qValue.d.p, db->common.d.p, db->firstWord.d.p, db->score.d.p};
    SIND_TRY(sind::launch_bowdb_query(a, db->capSlots, db->capWords, Q, s));
    SIND_TRY(db->common.down(Q * cs, s)); SIND_TRY(db->firstWord.down(Q * cs, s)); SIND_TRY(db->score.down(Q * cs, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < Q; i++) {
        std::memcpy(q[i].common, &db->common.h[i * cs], cs * sizeof(int)); std::memcpy(q[i].first_word, &db->firstWord.h[i * cs], cs * sizeof(int));
        std::memcpy(q[i].score, &db->score.h[i * cs], cs * sizeof(float));
    }
    return SIND_OK;
}

}  // extern "C"
