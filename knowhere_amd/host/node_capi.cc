// knowhere_amd/host/node_capi.cc -- a C view of the IndexNode (IndexFactory::Create / Index::Build /
// Search / Serialize / Deserialize), so that non-C++ hosts and the Python tests can drive the plugin
// exactly as Knowhere callers do.  Config is passed as "key=value;key=value" with the reference's key
// names (include/knowhere/comp/index_param.h:100-180): integers, true/false, or strings.
#include "hip_index_node.h"

#include <cstdlib>
#include <cstring>

using namespace knowhere;

extern "C" void knhip_host_normalize_rows(float* x, int64_t n, int64_t d, float* norms);  // hip_index_node.cc
extern "C" int32_t knhip_host_last_placement(int32_t* out, int32_t cap);                  // hip_index_node.cc

namespace {
thread_local std::string g_err;

Json ParseConfig(const char* s) {
    Json j;
    std::string str = s ? s : "";
    size_t pos = 0;
    while (pos < str.size()) {
        size_t end = str.find(';', pos);
        if (end == std::string::npos) end = str.size();
        const std::string kv = str.substr(pos, end - pos);
        pos = end + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        char* e = nullptr;
        const long long iv = std::strtoll(v.c_str(), &e, 10);
        if (v == "true" || v == "false") {
            j[k] = (v == "true");
        } else if (!v.empty() && e && *e == 0) {
            j[k] = (int64_t)iv;
        } else {
            char* e2 = nullptr;
            const double dv = std::strtod(v.c_str(), &e2);
            if (!v.empty() && e2 && *e2 == 0) j[k] = dv;
            else j[k] = v;
        }
    }
    return j;
}

struct Handle {
    Index<IndexNode> idx;
};
// the iterators of one Index::AnnIterator call
struct IterHandle {
    std::vector<IndexNode::IteratorPtr> its;
};
}  // namespace

extern "C" {

const char* knhip_node_last_error() { return g_err.c_str(); }

// IndexFactory::Instance().Create<fp32>(name, version); nullptr if the name is not registered
void* knhip_node_create(const char* name) {
    auto r = IndexFactory::Instance().Create<fp32>(name, Version::GetCurrentVersion().VersionNumber());
    if (!r.has_value()) {
        g_err = r.what();
        return nullptr;
    }
    return new Handle{r.value()};
}

void knhip_node_destroy(void* h) { delete static_cast<Handle*>(h); }

// Index::Build (= Train + Add); returns the Status value (0 = success)
int knhip_node_build(void* h, const float* x, int64_t rows, int64_t dim, const char* cfg) {
    auto ds = GenDataSet(rows, dim, x);
    return (int)static_cast<Handle*>(h)->idx.Build(ds, ParseConfig(cfg));
}

// Index::Search; ids/dist receive nq * k results.  bitset may be null.
int knhip_node_search(void* h, const float* q, int64_t nq, int64_t dim, const char* cfg, const uint8_t* bitset,
                      int64_t nbits, int64_t k, int64_t* ids, float* dist) {
    auto ds = GenDataSet(nq, dim, q);
    auto r = static_cast<Handle*>(h)->idx.Search(ds, ParseConfig(cfg), bitset ? BitsetView(bitset, (size_t)nbits) : BitsetView());
    if (!r.has_value()) {
        g_err = r.what();
        return (int)r.error();
    }
    std::memcpy(ids, r.value()->GetIds(), sizeof(int64_t) * nq * k);
    std::memcpy(dist, r.value()->GetDistance(), sizeof(float) * nq * k);
    return 0;
}

// Index::Serialize: copies the single blob of the BinarySet; returns its size (also when cap is too
// small) or -status.
int64_t knhip_node_serialize(void* h, uint8_t* out, int64_t cap) {
    BinarySet bs;
    auto& idx = static_cast<Handle*>(h)->idx;
    Status s = idx.Serialize(bs);
    if (s != Status::success) return -(int64_t)s;
    auto b = bs.GetByName(idx.Type());
    if (!b) return -(int64_t)Status::invalid_binary_set;
    if (b->size <= cap) std::memcpy(out, b->data.get(), (size_t)b->size);
    return b->size;
}

// Index::Deserialize from a BinarySet holding `data` under `key` (e.g. "IVF_PQ" for a CPU-built index)
int knhip_node_deserialize(void* h, const char* key, const uint8_t* data, int64_t size, const char* cfg) {
    BinarySet bs;
    std::shared_ptr<uint8_t[]> copy(new uint8_t[size]);
    std::memcpy(copy.get(), data, (size_t)size);
    bs.Append(key, copy, size);
    return (int)static_cast<Handle*>(h)->idx.Deserialize(bs, ParseConfig(cfg));
}

// Index::RangeSearch: lims[nq + 1]; *ids / *dist are malloc'ed copies (release with free())
int knhip_node_range_search(void* h, const float* q, int64_t nq, int64_t dim, const char* cfg, const uint8_t* bitset,
                            int64_t nbits, int64_t* lims, int64_t** ids, float** dist) {
    auto ds = GenDataSet(nq, dim, q);
    auto r = static_cast<Handle*>(h)->idx.RangeSearch(ds, ParseConfig(cfg),
                                                      bitset ? BitsetView(bitset, (size_t)nbits) : BitsetView());
    if (!r.has_value()) {
        g_err = r.what();
        return (int)r.error();
    }
    const size_t* l = r.value()->GetLims();
    for (int64_t i = 0; i <= nq; i++) lims[i] = (int64_t)l[i];
    const size_t n = l[nq];
    *ids = static_cast<int64_t*>(std::malloc(sizeof(int64_t) * (n + 1)));
    *dist = static_cast<float*>(std::malloc(sizeof(float) * (n + 1)));
    std::memcpy(*ids, r.value()->GetIds(), sizeof(int64_t) * n);
    std::memcpy(*dist, r.value()->GetDistance(), sizeof(float) * n);
    return 0;
}

// Index::AnnIterator: one iterator per query row behind *out (release with knhip_node_iter_destroy).  The query and bitset
// buffers may be released as soon as this returns.  Returns the Status value (0 = success).
int knhip_node_iter_create(void* h, const float* q, int64_t nq, int64_t dim, const char* cfg, const uint8_t* bitset,
                           int64_t nbits, void** out) {
    *out = nullptr;
    auto ds = GenDataSet(nq, dim, q);
    auto r = static_cast<Handle*>(h)->idx.AnnIterator(ds, ParseConfig(cfg),
                                                      bitset ? BitsetView(bitset, (size_t)nbits) : BitsetView());
    if (!r.has_value()) {
        g_err = r.what();
        return (int)r.error();
    }
    *out = new IterHandle{r.value()};
    return 0;
}

// iterator->Next() of query row i, up to n times: ids / dist receive the results, *got their number; the first failing
// Next() ends the page and its Status is returned (past the end: the reference's knowhere_inner_error)
int knhip_node_iter_next(void* it, int64_t i, int64_t n, int64_t* ids, float* dist, int64_t* got) {
    auto* ih = static_cast<IterHandle*>(it);
    *got = 0;
    if (i < 0 || (size_t)i >= ih->its.size()) return (int)Status::invalid_args;
    for (int64_t j = 0; j < n; j++) {
        auto r = ih->its[(size_t)i]->Next();
        if (!r.has_value()) {
            g_err = r.what();
            return (int)r.error();
        }
        ids[j] = r.value().first;
        dist[j] = r.value().second;
        *got = j + 1;
    }
    return 0;
}

// iterator->HasNext(): 1 / 0, or -Status
int knhip_node_iter_has_next(void* it, int64_t i) {
    auto* ih = static_cast<IterHandle*>(it);
    if (i < 0 || (size_t)i >= ih->its.size()) return -(int)Status::invalid_args;
    auto r = ih->its[(size_t)i]->HasNext();
    if (!r.has_value()) {
        g_err = r.what();
        return -(int)r.error();
    }
    return r.value() ? 1 : 0;
}

void knhip_node_iter_destroy(void* it) { delete static_cast<IterHandle*>(it); }

// the node's NormalizeVec restatement on n rows in place (norms may be null): test hook for the bitwise check against
// knowhere::NormalizeVecs (src/common/utils.cc:60-93)
void knhip_node_normalize_rows(float* x, int64_t n, int64_t d, float* norms) { knhip_host_normalize_rows(x, n, d, norms); }

// Index::Train / Index::Add separately (Build = both): repeated Add is how a growing segment is fed
int knhip_node_train(void* h, const float* x, int64_t rows, int64_t dim, const char* cfg) {
    auto ds = GenDataSet(rows, dim, x);
    return (int)static_cast<Handle*>(h)->idx.Train(ds, ParseConfig(cfg));
}
int knhip_node_add(void* h, const float* x, int64_t rows, int64_t dim, const char* cfg) {
    auto ds = GenDataSet(rows, dim, x);
    return (int)static_cast<Handle*>(h)->idx.Add(ds, ParseConfig(cfg));
}

// Index::GetVectorByIds: out receives n * dim floats
int knhip_node_get_vectors(void* h, const int64_t* ids, int64_t n, int64_t dim, float* out) {
    auto ds = GenIdsDataSet(n, ids);
    auto r = static_cast<Handle*>(h)->idx.GetVectorByIds(ds);
    if (!r.has_value()) {
        g_err = r.what();
        return (int)r.error();
    }
    std::memcpy(out, r.value()->GetTensor(), sizeof(float) * (size_t)(n * dim));
    return 0;
}

// Index::CalcDistByIDs: q [nq][dim], labels [n_labels] (public ids; identity unless an id map is installed); out receives
// nq * n_labels floats.  Returns the Status (0 = success), the text through knhip_node_last_error.
int knhip_node_calc_dist_by_ids(void* h, const float* q, int64_t nq, int64_t dim, const int64_t* labels, int64_t n_labels,
                                int32_t is_cosine, float* out) {
    auto ds = GenDataSet(nq, dim, q);
    auto r = static_cast<Handle*>(h)->idx.CalcDistByIDs(ds, BitsetView(), labels, (size_t)n_labels, is_cosine != 0);
    if (!r.has_value()) {
        g_err = r.what();
        return (int)r.error();
    }
    if (r.value()->GetRows() != nq || r.value()->GetDim() != n_labels || r.value()->GetIds() != nullptr) {
        g_err = "CalcDistByIDs: result shape is not rows = nq, dim = labels_len, distances only";
        return (int)knowhere::Status::knowhere_inner_error;
    }
    if (nq * n_labels > 0) {
        std::memcpy(out, r.value()->GetDistance(), sizeof(float) * (size_t)(nq * n_labels));
    }
    return 0;
}

// An embedding-list index in two steps, as IndexNode::BuildEmbList (src/index/index_node.cc:453-508) does for the tokenann
// strategy: Train with the metric's sub metric on all the vectors, then IndexNode::AddEmbList with the documents' offsets
// (lims[0] = 0 .. lims[ndocs] = rows) under the emb_list metric itself.  Returns the Status value (0 = success).
int knhip_node_build_emb_list(void* h, const float* x, int64_t rows, int64_t dim, const int64_t* lims, int64_t ndocs,
                              const char* cfg) {
    auto* node = static_cast<Handle*>(h)->idx.Node();
    const Status st = Index<IndexNode>::Guard([&] {
        Json j = ParseConfig(cfg);
        auto ds = GenDataSet(rows, dim, x);
        std::string msg;
        std::shared_ptr<Config> add_cfg = node->CreateConfig();
        Status s = Index<IndexNode>::LoadConfig(static_cast<BaseConfig*>(add_cfg.get()), j, PARAM_TYPE::TRAIN, &msg);
        if (s != Status::success) {
            g_err = msg;
            return s;
        }
        const std::string metric = static_cast<BaseConfig*>(add_cfg.get())->metric_type.value_or("");
        const char* sub = HipEmbListSubMetric(metric);
        if (sub == nullptr) {
            g_err = "invalid metric type for emb_list: " + metric;
            return Status::emb_list_inner_error;
        }
        j["metric_type"] = sub;
        std::shared_ptr<Config> train_cfg = node->CreateConfig();
        s = Index<IndexNode>::LoadConfig(static_cast<BaseConfig*>(train_cfg.get()), j, PARAM_TYPE::TRAIN, &msg);
        if (s != Status::success) {
            g_err = msg;
            return s;
        }
        RETURN_IF_ERROR(node->Train(ds, train_cfg, true));
        const std::vector<size_t> l(lims, lims + ndocs + 1);
        return node->AddEmbList(ds, add_cfg, l.data(), (size_t)rows, true);
    });
    return (int)st;
}

// IndexNode::SearchEmbList: q [nqv][dim] holds nel query lists, list e = rows q_lims[e] .. q_lims[e + 1] - 1 (q_lims[nel] =
// nqv); ids / scores receive nel * k results (k from the config).  bitset (over vector ids) may be null.
int knhip_node_search_emb_list(void* h, const float* q, int64_t nqv, int64_t dim, const int64_t* q_lims, int64_t nel,
                               const char* cfg, const uint8_t* bitset, int64_t nbits, int64_t* ids, float* scores) {
    auto* node = static_cast<Handle*>(h)->idx.Node();
    if (!q_lims || nel < 0 || q_lims[0] != 0 || q_lims[nel] != nqv) {
        // (IndexNode::SearchEmbList reads the offsets up to the entry that equals the number of rows)
        g_err = "SearchEmbList: the query offsets must run from 0 to the number of query vectors";
        return (int)Status::invalid_args;
    }
    try {
        auto c = node->CreateConfig();
        std::string msg;
        const Status s = Index<IndexNode>::LoadConfig(c.get(), ParseConfig(cfg), PARAM_TYPE::SEARCH, &msg);
        if (s != Status::success) {
            g_err = msg;
            return (int)s;
        }
        const int64_t k = c->k.value();
        const std::vector<size_t> l(q_lims, q_lims + nel + 1);
        auto ds = GenDataSet(nqv, dim, q);
        ds->SetLims(l.data());  // (not owned: GenDataSet's datasets own nothing)
        auto r = node->SearchEmbList(ds, std::move(c), node->PrepareBitset(bitset ? BitsetView(bitset, (size_t)nbits) : BitsetView()),
                                     nullptr);
        if (!r.has_value()) {
            g_err = r.what();
            return (int)r.error();
        }
        if (r.value()->GetRows() != nel || r.value()->GetDim() != k) {
            g_err = "SearchEmbList: result shape is not rows = number of query lists, dim = k";
            return (int)Status::knowhere_inner_error;
        }
        std::memcpy(ids, r.value()->GetIds(), sizeof(int64_t) * (size_t)(nel * k));
        std::memcpy(scores, r.value()->GetDistance(), sizeof(float) * (size_t)(nel * k));
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return (int)Status::knowhere_inner_error;
    }
}

// where the index built / loaded last on the calling thread was placed (device ordinals in shard order): test hook
int32_t knhip_node_last_placement(int32_t* out, int32_t cap) { return knhip_host_last_placement(out, cap); }

// Index::Size: the HBM the index holds over all its devices (knhip_index_device_bytes of every shard + the refine stores)
int64_t knhip_node_device_bytes(void* h) { return static_cast<Handle*>(h)->idx.Size(); }
int64_t knhip_node_count(void* h) { return static_cast<Handle*>(h)->idx.Count(); }
int64_t knhip_node_dim(void* h) { return static_cast<Handle*>(h)->idx.Dim(); }

}  // extern "C"
